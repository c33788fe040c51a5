// warp_band.hpp — the affine warp behind the fixed output size (jpgpu_batch_create_warped): every image's u8 result
// R of out_w x out_h, as the same batch without a warp writes it, is read through six coefficients m[0..5] — Pillow's
// Image.transform(size, Image.AFFINE, m, resample, fillcolor=): the inverse map, output pixel -> source position — and written as u8
// pixels or as the normalised CHW tensor of tensor_band.hpp:
//     out(Y, X, c)  = Warp( flip ? mirror_columns(R) : R )(Y, X, c)
//     elem(c, Y, X) = T[c][ out(Y, X, c) ]
// Three bodies, one per image (WarpJob::kind), each the statement of what Pillow computes:
//   N     NEAREST, m[1] != 0 || m[3] != 0: 16.16 fixed point, a[] made on the host (warp_fix).
//   N-sep NEAREST, m[1] == 0 && m[3] == 0: an index table per axis, sequential sums of doubles made on the host (warp_nearest_axis).
//   B     BILINEAR: IEEE double, one rounding per operation (wp_mul / wp_add: no fused multiply-add), the result truncated.
// One lane per output pixel, X fastest: the tensor's plane stores and the u8 stores of a wave are contiguous; the source is read straight
// from the intermediate arena (an image of 224 x 224 x 3 is 150 kB: L2).  No LDS.  A flip mirrors the column READ from R.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__) || defined(JPGPU_HOST_EMULATION)
#define JPGPU_WP_DEVICE_BODY 1
#include "pixel_math.hpp"
#endif

namespace jpgpu {

constexpr uint32_t WP_NEAREST = 0, WP_BILINEAR = 1;          // JPGPU_WARP_*
constexpr uint32_t WP_KIND_N = 0, WP_KIND_NSEP = 1, WP_KIND_B = 2;
constexpr uint32_t WP_NT = 256;                              // lanes of a workgroup = output pixels of a tile
constexpr double WP_MAX_COEF = 16000.0, WP_MAX_POS = 32000.0;

// One image of the launch.  src: R, h x w x nc bytes; dst: the image's pixels (h x w x nc bytes) or its tensor (nc planes of `plane`
// elements); tab: where the image's N-sep tables lie in the launch's table block (w entries for X, then h for Y).
struct WarpJob {
    const uint8_t *src;
    void *dst;
    double m[6];
    int32_t a[6];
    uint32_t w, h, nc, kind, flip;
    uint32_t fill;  // wfill[c] in byte c
    uint32_t plane;
    uint32_t tab;
};

// What a matrix must be for an output of ow x oh: finite, |m0|, |m1|, |m3|, |m4| <= 16000, and the source position of every corner of
// the output within +-32000 — every fixed-point sum of rule N then fits 32 bits (the pixel centres lie inside the corners' hull).
inline bool warp_check(const double *m, uint32_t ow, uint32_t oh) {
    for (int k = 0; k < 6; k++)
        if (!(fabs(m[k]) <= 1.7976931348623157e308)) return false;  // (NaN compares false)
    if (fabs(m[0]) > WP_MAX_COEF || fabs(m[1]) > WP_MAX_COEF || fabs(m[3]) > WP_MAX_COEF || fabs(m[4]) > WP_MAX_COEF) return false;
    const double xs[2] = {0.0, (double)ow}, ys[2] = {0.0, (double)oh};
    for (int cy = 0; cy < 2; cy++)
        for (int cx = 0; cx < 2; cx++) {
            const double ax = xs[cx] * m[0], bx = ys[cy] * m[1], sx = ax + bx, px = sx + m[2];
            const double ay = xs[cx] * m[3], by = ys[cy] * m[4], sy = ay + by, py = sy + m[5];
            if (!(fabs(px) <= WP_MAX_POS) || !(fabs(py) <= WP_MAX_POS)) return false;
        }
    return true;
}

// FIX of Pillow's Geometry.c; |v| <= 32000 by warp_check
inline int32_t warp_fix(double v) {
    const double s = v * 65536.0, r = s + 0.5;
    return (int32_t)floor(r);
}

// The N-sep index table of one axis: the source index of output pixel X at scale a and offset b, a sequential sum of doubles; -1 left
// of the source (an index at or beyond the source's size is for the reader to refuse).  Arguments of any size: a position that no int
// holds gives INT32_MAX, one that is no number -1.
inline void warp_nearest_axis(double a, double b, uint32_t out_size, int32_t *idx) {
    const double half = a * 0.5;
    double xo = b + half;
    for (uint32_t x = 0; x < out_size; x++) {
        idx[x] = !(xo >= 0.0) ? -1 : (xo >= 2147483647.0 ? 2147483647 : (int32_t)xo);
        xo = xo + a;
    }
}

// The matrix into a job (the caller has checked it): the kind under `filter`, the fixed-point coefficients of rule N, the image's two
// N-sep tables into tab[0, w) and tab[w, w + h).
inline void warp_job_matrix(WarpJob &j, const double *m, uint32_t filter, int32_t *tab) {
    for (int k = 0; k < 6; k++) j.m[k] = m[k], j.a[k] = 0;
    j.kind = filter == WP_BILINEAR ? WP_KIND_B : ((m[1] == 0.0 && m[3] == 0.0) ? WP_KIND_NSEP : WP_KIND_N);
    if (j.kind == WP_KIND_N) {
        j.a[0] = warp_fix(m[0]), j.a[1] = warp_fix(m[1]), j.a[3] = warp_fix(m[3]), j.a[4] = warp_fix(m[4]);
        const double x0 = m[0] * 0.5, x1 = m[2] + x0, x2 = m[1] * 0.5, x3 = x1 + x2;
        const double y0 = m[3] * 0.5, y1 = m[5] + y0, y2 = m[4] * 0.5, y3 = y1 + y2;
        j.a[2] = warp_fix(x3), j.a[5] = warp_fix(y3);
    }
    if (j.kind == WP_KIND_NSEP) {
        warp_nearest_axis(m[0], m[2], j.w, tab);
        warp_nearest_axis(m[4], m[5], j.h, tab + j.w);
    }
}

#ifdef JPGPU_WP_DEVICE_BODY
// IEEE double, rounded once per operation.  hipcc contracts a * b + c into a fused multiply-add by default, across statements and through
// __dmul_rn / __dadd_rn (plain products and sums in its headers): the pragma takes the permission from the operation itself, and the
// kernels' disassembly must show neither v_fma_f64 nor v_fmac_f64 (profiles/warp/).  The host's versions, for the emulation, store the
// result before it is used.
static __host__ __device__ __forceinline__ double wp_mul(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
    return a * b;
#else
    volatile double r = a * b;
    return r;
#endif
}
static __host__ __device__ __forceinline__ double wp_add(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
    return a + b;
#else
    volatile double r = a + b;
    return r;
#endif
}

struct AffBand {
    // the four taps of rule B: columns x0, x1 of rows r0 and r1 (two == false: one row), the weights
    struct Taps {
        uint32_t x0, x1, r0, r1;
        bool two;
        double dx, dy;
    };

    static __device__ __forceinline__ uint32_t tiles_of(uint32_t w, uint32_t h) { return (w * h + WP_NT - 1u) / WP_NT; }

    // rule N: the sums wrap in 32 bits on the way and fit at the end (warp_check)
    static __device__ __forceinline__ bool pos_n(const WarpJob &j, uint32_t X, uint32_t Y, uint32_t &xi, uint32_t &yi) {
        const int32_t x = (int32_t)((uint32_t)j.a[2] + X * (uint32_t)j.a[0] + Y * (uint32_t)j.a[1]) >> 16;
        const int32_t y = (int32_t)((uint32_t)j.a[5] + X * (uint32_t)j.a[3] + Y * (uint32_t)j.a[4]) >> 16;
        xi = (uint32_t)x, yi = (uint32_t)y;
        return x >= 0 && x < (int32_t)j.w && y >= 0 && y < (int32_t)j.h;
    }
    static __device__ __forceinline__ bool pos_nsep(const WarpJob &j, const JP_GLOBAL int32_t *tab, uint32_t X, uint32_t Y, uint32_t &xi, uint32_t &yi) {
        const int32_t x = tab[j.tab + X], y = tab[j.tab + j.w + Y];
        xi = (uint32_t)x, yi = (uint32_t)y;
        return x >= 0 && x < (int32_t)j.w && y >= 0 && y < (int32_t)j.h;
    }
    static __device__ __forceinline__ bool pos_b(const WarpJob &j, uint32_t X, uint32_t Y, Taps &t) {
        const double xin = (double)X + 0.5, yin = (double)Y + 0.5;  // (exact)
        double xo = wp_add(wp_add(wp_mul(j.m[0], xin), wp_mul(j.m[1], yin)), j.m[2]);
        double yo = wp_add(wp_add(wp_mul(j.m[3], xin), wp_mul(j.m[4], yin)), j.m[5]);
        if (xo < 0.0 || xo >= (double)j.w || yo < 0.0 || yo >= (double)j.h) return false;
        xo = wp_add(xo, -0.5), yo = wp_add(yo, -0.5);
        const int32_t x = xo < 0.0 ? -1 : (int32_t)xo, y = yo < 0.0 ? -1 : (int32_t)yo;  // floor: xo >= -0.5
        t.dx = wp_add(xo, -(double)x), t.dy = wp_add(yo, -(double)y);
        const int32_t w1 = (int32_t)j.w - 1, h1 = (int32_t)j.h - 1;
        t.x0 = (uint32_t)(x < 0 ? 0 : x), t.x1 = (uint32_t)(x + 1 > w1 ? w1 : x + 1);
        t.r0 = (uint32_t)(y < 0 ? 0 : y);
        t.two = y + 1 <= h1;  // (y + 1 >= 0 always)
        t.r1 = t.two ? (uint32_t)(y + 1) : t.r0;
        return true;
    }
    static __device__ __forceinline__ uint32_t sample_b(const Taps &t, uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11) {
        const double v1 = wp_add((double)p00, wp_mul((double)((int32_t)p01 - (int32_t)p00), t.dx));
        double v2 = v1;
        if (t.two) v2 = wp_add((double)p10, wp_mul((double)((int32_t)p11 - (int32_t)p10), t.dx));
        const double v = wp_add(v1, wp_mul(wp_add(v2, -v1), t.dy));
        return (uint32_t)(int32_t)v & 255u;  // truncated; v lies in 0..255
    }

    // Output pixel p = Y * w + X of the job -> its nc bytes in bytes 0.. of the result (outside the source: the fill)
    static __device__ __forceinline__ uint32_t pixel(const WarpJob &j, const JP_GLOBAL int32_t *tab, uint32_t p) {
        const uint32_t w = j.w, nc = j.nc, Y = p / w, X = p - Y * w;
        const JP_GLOBAL uint8_t *src = (const JP_GLOBAL uint8_t *)j.src;
        uint32_t px = j.fill;
        if (j.kind == WP_KIND_B) {  // (uniform)
            Taps t;
            if (!pos_b(j, X, Y, t)) return px;
            const uint32_t c0 = j.flip ? w - 1u - t.x0 : t.x0, c1 = j.flip ? w - 1u - t.x1 : t.x1;
            const JP_GLOBAL uint8_t *q00 = src + ((size_t)t.r0 * w + c0) * nc, *q01 = src + ((size_t)t.r0 * w + c1) * nc;
            const JP_GLOBAL uint8_t *q10 = src + ((size_t)t.r1 * w + c0) * nc, *q11 = src + ((size_t)t.r1 * w + c1) * nc;
            px = 0u;
            for (uint32_t c = 0; c < nc; c++) px |= sample_b(t, q00[c], q01[c], q10[c], q11[c]) << (8u * c);
            return px;
        }
        uint32_t xi, yi;
        const bool in = j.kind == WP_KIND_N ? pos_n(j, X, Y, xi, yi) : pos_nsep(j, tab, X, Y, xi, yi);
        if (!in) return px;
        const JP_GLOBAL uint8_t *q = src + ((size_t)yi * w + (j.flip ? w - 1u - xi : xi)) * nc;
        px = 0u;
        for (uint32_t c = 0; c < nc; c++) px |= (uint32_t)q[c] << (8u * c);
        return px;
    }

    // lane `tid` of tile `tile`: its pixel, stored as bytes ...
    static __device__ __forceinline__ void lane_u8(const WarpJob &j, const JP_GLOBAL int32_t *tab, uint32_t tile, uint32_t tid) {
        const uint32_t p = tile * WP_NT + tid, nc = j.nc;
        if (p >= j.w * j.h) return;
        const uint32_t px = pixel(j, tab, p);
        JP_GLOBAL uint8_t *dst = (JP_GLOBAL uint8_t *)j.dst + (size_t)p * nc;
        if (nc == 4u) {  // (the image's base is 256-byte aligned)
            *reinterpret_cast<JP_GLOBAL uint32_t *>(dst) = px;
            return;
        }
        for (uint32_t c = 0; c < nc; c++) dst[c] = (uint8_t)(px >> (8u * c));
    }
    // ... or as one element per plane, looked up in T (E: the element's bits)
    template <class E>
    static __device__ __forceinline__ void lane_tensor(const WarpJob &j, const JP_GLOBAL int32_t *tab, const JP_GLOBAL E *T, uint32_t tile, uint32_t tid) {
        const uint32_t p = tile * WP_NT + tid, nc = j.nc;
        if (p >= j.w * j.h) return;
        const uint32_t px = pixel(j, tab, p);
        JP_GLOBAL E *dst = (JP_GLOBAL E *)j.dst;
        for (uint32_t c = 0; c < nc; c++) dst[(size_t)c * j.plane + p] = T[c * 256u + ((px >> (8u * c)) & 255u)];
    }
};
#endif  // JPGPU_WP_DEVICE_BODY

}  // namespace jpgpu

#if defined(__HIP__) && !defined(JPGPU_HOST_EMULATION)
namespace jpgpu {
// warp.hip: n_images jobs of at most max_tiles tiles each, their N-sep tables in d_tab; elem_bytes 0: u8 pixels, 2 / 4: tensors through
// the table d_ttab (4 x 256 elements)
hipError_t launch_warp(const WarpJob *d_jobs, const int32_t *d_tab, const void *d_ttab, uint32_t elem_bytes, uint32_t n_images, uint32_t max_tiles,
                       hipStream_t stream);
}  // namespace jpgpu
#endif
