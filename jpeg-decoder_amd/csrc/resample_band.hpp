// resample_band.hpp — every image of a batch resampled to one output size (jpgpu_batch_create_resized) in ONE launch: the pixels the
// batch's other kernels wrote (an image's window, or its whole output) in, out_h x out_w x nc bytes out, interleaved and packed.
//
// The arithmetic is the 8-bit integer bilinear resample with antialiasing of Pillow's Image.resize(size, BILINEAR) on the cropped
// image (include/jpgpu.h): per axis a table of (xmin, n) and n 22-bit integer weights per output index, made on
// the host in IEEE double (resample_coefficients below, = jpgpu_resample_coefficients); one pass is
//     out = clamp((2^21 + sum p[xmin + x] * k[x]) >> 22, 0, 255)      (32-bit integers; the sum stays below 2^31)
// the horizontal pass first, rounded to u8, the vertical pass on its result.  The device does integer work only.
//
//   1. planner (resample_plan, no HIP dependency: tests/emu runs it): a workgroup owns one image and a band of `rb` output rows.  The
//      band's bytes are one run of the packed output (rows of out_w * nc bytes follow each other), cut into destination dwords.  The
//      source rows a band needs ([ymin of its first row, ymax of its last)) go through LDS `cap_rows` at a time; `rb` is the largest
//      band whose rows fit in one such chunk (RS_MAX_LDS).  A single output row whose support does not fit takes several chunks:
//      RS_NT destination dwords at a time, every lane keeps the four sums of its dword in registers over the chunks.
//   2. horizontal pass (RBand::hpass): one lane per (RS_HROWS source rows of the chunk, output column); the taps' bytes come from global memory
//      as aligned dwords whatever the row's alignment (window rows of w * nc bytes start anywhere), neighbouring lanes read
//      neighbouring / overlapping spans.  u8 rows of out_w * nc bytes (pitch rounded up to 4) into LDS.
//   3. vertical pass (RBand::vpass): one lane per destination dword; where the dword's four bytes lie in one output row at a multiple
//      of four (always when out_w * nc is one) the taps are aligned LDS dword reads, else byte reads.  Sums are exact in int32, so
//      chunks add up in any order.
//   4. store: whole aligned dwords; the first / last dword of a band that it shares with its neighbour byte by byte.
//   5. RGB output (JPGPU_BATCH_RGB_OUTPUT): a job with src_nc = 1 / 4 has a gray / CMYK source and nc = 3; its
//      horizontal pass (RBand::hpass_walk<1> / hpass_cmyk) converts the source pixels and leaves the three-channel rows in LDS that 2.
//      leaves for a three-channel source — 1., 3. and 4. run unchanged with nc = 3.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

// (the tables and the planner need no HIP: image_job.cpp, a plain C++ translation unit, takes them from here)
#if defined(__HIP__) || defined(JPGPU_HOST_EMULATION)
#define JPGPU_RS_DEVICE_BODY 1
#include "pixel_math.hpp"
#endif

namespace jpgpu {

constexpr uint32_t RS_NT = 256;               // lanes per workgroup
constexpr uint32_t RS_HROWS = 4;              // source rows a lane takes through the horizontal pass side by side (one column: the taps' weights
                                              // are loaded once for them, their loads are independent of one another)
constexpr uint32_t RS_MAX_LDS = 32u * 1024u;  // 5 workgroups share a CU's 160 kB
constexpr uint32_t RS_MAX_OUT = 2048;         // largest output width / height
constexpr uint32_t RS_PRECISION_BITS = 22;

// The filters of DESIGN.md §4.15 (JPGPU_FILTER_* of include/jpgpu.h): Pillow's BILINEAR, BOX, HAMMING, BICUBIC and LANCZOS.
constexpr uint32_t RS_FILTER_BILINEAR = 0, RS_FILTER_BOX = 1, RS_FILTER_HAMMING = 2, RS_FILTER_BICUBIC = 3, RS_FILTER_LANCZOS = 4, RS_FILTERS = 5;
inline double resample_filter_support(uint32_t filter) {
    return filter == RS_FILTER_BOX ? 0.5 : filter == RS_FILTER_BICUBIC ? 2.0 : filter == RS_FILTER_LANCZOS ? 3.0 : 1.0;
}
inline const char *resample_filter_name(uint32_t filter) {
    static const char *const names[RS_FILTERS] = {"bilinear", "box", "hamming", "bicubic", "lanczos"};
    return filter < RS_FILTERS ? names[filter] : "?";
}
// sin(pi x) / (pi x), one operation per statement
inline double resample_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    const double s = sin(x);
    return s / x;
}
// The filter's weight at the SIGNED argument x: IEEE double, libm's sin and cos, one operation per statement (nothing for a compiler
// to contract into an FMA) in the order of the statement in DESIGN.md §4.15.
inline double resample_filter_weight(uint32_t filter, double x) {
    if (filter == RS_FILTER_BOX) return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
    if (filter == RS_FILTER_LANCZOS) {
        if (!(-3.0 <= x && x < 3.0)) return 0.0;
        const double s1 = resample_sinc(x);
        const double x3 = x / 3.0;
        const double s3 = resample_sinc(x3);
        return s1 * s3;
    }
    if (x < 0.0) x = -x;
    if (filter == RS_FILTER_HAMMING) {
        if (x == 0.0) return 1.0;
        if (x >= 1.0) return 0.0;
        x = x * M_PI;
        const double s = sin(x);
        const double q = s / x;
        const double c = cos(x);
        double h = (double)0.46f * c;  // (the two constants are float literals promoted to double)
        h = (double)0.54f + h;
        return q * h;
    }
    if (filter == RS_FILTER_BICUBIC) {  // a = -0.5
        if (x < 1.0) {                  // ((a + 2) x - (a + 3)) x x + 1
            double v = 1.5 * x;
            v = v - 2.5;
            v = v * x;
            v = v * x;
            return v + 1.0;
        }
        if (x < 2.0) {  // (((x - 5) x + 8) x - 4) a
            double v = x - 5.0;
            v = v * x;
            v = v + 8.0;
            v = v * x;
            v = v - 4.0;
            return v * -0.5;
        }
        return 0.0;
    }
    return x < 1.0 ? 1.0 - x : 0.0;
}

// ksize of an axis: ceil(S_F * max(in / out, 1)) * 2 + 1
inline uint32_t resample_ksize_filtered(uint32_t filter, uint32_t in_size, uint32_t out_size) {
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = resample_filter_support(filter) * fs;
    uint32_t c = (uint32_t)support;
    if ((double)c < support) c++;
    return c * 2u + 1u;
}
inline uint32_t resample_ksize(uint32_t in_size, uint32_t out_size) { return resample_ksize_filtered(RS_FILTER_BILINEAR, in_size, out_size); }

// Entries [first, first + count) of the tables of one axis under a filter: bounds[2 i] = xmin, bounds[2 i + 1] = n,
// coefs[i * ksize + x] = k[x] (zero beyond n) belong to output index first + i.  IEEE double, the operations in the order of the
// statement in DESIGN.md §4.10 / §4.15 (one operation per statement: nothing for a compiler to contract).  Weights may be negative.
inline void resample_coefficients_range_filtered(uint32_t filter, uint32_t in_size, uint32_t out_size, uint32_t first, uint32_t count, int32_t *bounds,
                                                 int32_t *coefs, uint32_t ksize) {
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = resample_filter_support(filter) * fs;
    const double ss = 1.0 / fs;
    for (uint32_t i = 0; i < count; i++) {
        const uint32_t xx = first + i;
        const double center = ((double)xx + 0.5) * scale;
        int32_t xmin = (int32_t)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int32_t xmax = (int32_t)(center + support + 0.5);
        if (xmax > (int32_t)in_size) xmax = (int32_t)in_size;
        const int32_t n = xmax - xmin;
        int32_t *k = coefs + (size_t)i * ksize;
        double ww = 0.0;
        for (int32_t x = 0; x < n; x++) {
            double a = (double)(x + xmin) - center;
            a = a + 0.5;
            a = a * ss;
            const double w = resample_filter_weight(filter, a);
            ww = ww + w;
        }
        for (int32_t x = 0; x < (int32_t)ksize; x++) {
            if (x >= n) {
                k[x] = 0;
                continue;
            }
            double a = (double)(x + xmin) - center;
            a = a + 0.5;
            a = a * ss;
            const double w = resample_filter_weight(filter, a);
            double v = ww != 0.0 ? w / ww : w;
            v = v * (double)(1 << RS_PRECISION_BITS);
            k[x] = v < 0.0 ? (int32_t)(-0.5 + v) : (int32_t)(0.5 + v);
        }
        bounds[2 * i] = xmin, bounds[2 * i + 1] = n;
    }
}
inline void resample_coefficients_filtered(uint32_t filter, uint32_t in_size, uint32_t out_size, int32_t *bounds, int32_t *coefs, uint32_t ksize) {
    resample_coefficients_range_filtered(filter, in_size, out_size, 0u, out_size, bounds, coefs, ksize);
}
// The tables of one axis under BILINEAR (§4.10): filter 0 of the above.
inline void resample_coefficients(uint32_t in_size, uint32_t out_size, int32_t *bounds, int32_t *coefs, uint32_t ksize) {
    resample_coefficients_range_filtered(RS_FILTER_BILINEAR, in_size, out_size, 0u, out_size, bounds, coefs, ksize);
}

// One image of the launch.  Table offsets count int32 words from the launch's table base.
struct ResampleJob {
    const uint8_t *src;  // in_h rows of in_w * nc bytes, packed
    uint8_t *dst;        // out_h rows of out_w * nc bytes, packed; 4-byte aligned
    uint32_t in_w, in_h, nc, out_w, out_h;
    uint32_t hb, hk, hks;  // horizontal bounds / coefficients / ksize
    uint32_t vb, vk, vks;  // vertical
    uint32_t rb, bands;    // output rows per band, bands
    uint32_t cap_rows;     // source rows per LDS chunk
    uint32_t pitch;        // LDS row pitch: out_w * nc rounded up to 4
    uint32_t lds_bytes;    // cap_rows * pitch
    uint32_t src_nc;       // 0: the source has nc channels.  1 / 4 (RGB output; nc is 3 then): the source has src_nc channels,
                           // the horizontal pass converts them (RBand::hpass_walk<1> / hpass_cmyk) and leaves three-channel rows in LDS
};

// Plans the bands of a job whose sizes and table offsets are set and whose tables (`tab`, host copy) are filled.  False for sizes the
// kernel does not run (the batch refuses them before).
inline bool resample_plan(ResampleJob &j, const int32_t *tab, uint32_t lds_cap = RS_MAX_LDS, uint32_t rb_cap = 64u) {
    if (j.src_nc != 0 && (j.nc != 3 || (j.src_nc != 1 && j.src_nc != 4))) return false;
    if (j.nc == 0 || j.nc > 4 || j.in_w == 0 || j.in_h == 0 || j.out_w == 0 || j.out_h == 0 || j.out_w > RS_MAX_OUT || j.out_h > RS_MAX_OUT) return false;
    const uint32_t rowb = j.out_w * j.nc;
    j.pitch = (rowb + 3u) & ~3u;
    if (lds_cap > RS_MAX_LDS) lds_cap = RS_MAX_LDS;
    j.cap_rows = lds_cap / j.pitch;
    if (j.cap_rows == 0) return false;
    if (j.cap_rows > j.in_h) j.cap_rows = j.in_h;
    j.lds_bytes = j.cap_rows * j.pitch;
    const int32_t *vb = tab + j.vb;
    uint32_t rb = rb_cap ? rb_cap : 1u;
    if (rb > j.out_h) rb = j.out_h;
    for (; rb > 1u; rb--) {  // the largest band whose source rows fit in one chunk, for every band
        bool ok = true;
        for (uint32_t r0 = 0; r0 < j.out_h && ok; r0 += rb) {
            const uint32_t r1 = r0 + rb < j.out_h ? r0 + rb : j.out_h;
            const uint32_t s0 = (uint32_t)vb[2 * r0], s1 = (uint32_t)(vb[2 * (r1 - 1u)] + vb[2 * (r1 - 1u) + 1]);
            ok = s1 - s0 <= j.cap_rows;
        }
        if (ok) break;
    }
    j.rb = rb;
    j.bands = (j.out_h + rb - 1u) / rb;
    return true;
}

// ---- runs of bands.  Under wide filters the source rows of neighbouring bands overlap, and every band passes the rows
// it shares with its neighbour through the horizontal pass again.  A workgroup that takes a run of `bpr` consecutive bands keeps the
// shared rows in LDS instead (RBand::roll_*).  Planner side: which plans may take the route, and what they would save. ----
constexpr uint32_t RS_ROLL_DW = 8;  // dwords a lane carries through one slab of the move
// Σ band source rows and the source rows the image reads; false where a band takes more than one chunk (those keep their bands)
inline bool resample_band_rows(const ResampleJob &j, const int32_t *tab, uint64_t &passed, uint32_t &read) {
    const int32_t *vb = tab + j.vb;
    passed = 0;
    for (uint32_t r0 = 0; r0 < j.out_h; r0 += j.rb) {
        const uint32_t r1 = r0 + j.rb < j.out_h ? r0 + j.rb : j.out_h;
        const uint32_t s0 = (uint32_t)vb[2 * r0], s1 = (uint32_t)(vb[2 * (r1 - 1u)] + vb[2 * (r1 - 1u) + 1]);
        if (s1 - s0 > j.cap_rows) return false;
        passed += s1 - s0;
    }
    read = (uint32_t)(vb[2 * (j.out_h - 1u)] + vb[2 * (j.out_h - 1u) + 1]) - (uint32_t)vb[0];
    return true;
}
// bands per run for a job under `filter` (0: the job keeps its bands).  `knob`: 0 the rule below; 1 never; 2 / 4 / 8 that many for every
// candidate (tools/filter_bench.py measures the routes against each other with it).  Candidates are BICUBIC and LANCZOS jobs of at
// least two one-chunk bands.  The rule is the measurement's (profiles/filters/filter_bench.json): plans whose redundancy
// (Σ band source rows / source rows read) exceeds 1.30 — 1.31 is the lowest that won by more than the band route's own spread, 1.21
// the highest that lost — with 8 bands per run where that still leaves four runs, else 4 (8 of 14 bands: two workgroups per image, 1.05-1.26 x).
constexpr uint32_t RS_ROLL_MIN_PERCENT = 130, RS_ROLL_LONG_BANDS = 32;
inline uint32_t resample_roll_bpr(const ResampleJob &j, const int32_t *tab, uint32_t filter, uint32_t knob) {
    if (knob == 1u || (filter != RS_FILTER_BICUBIC && filter != RS_FILTER_LANCZOS) || j.bands < 2u) return 0u;
    uint64_t passed;
    uint32_t read;
    if (!resample_band_rows(j, tab, passed, read)) return 0u;
    if (knob == 2u || knob == 4u || knob == 8u) return knob;
    return passed * 100u > (uint64_t)read * RS_ROLL_MIN_PERCENT ? (j.bands >= RS_ROLL_LONG_BANDS ? 8u : 4u) : 0u;
}

#ifdef JPGPU_RS_DEVICE_BODY
struct RBand {
    // the band's output rows [r0, r1) and its source rows [s0, s1)
    static __device__ __forceinline__ void rows_of(const ResampleJob &j, const JP_GLOBAL int32_t *tab, uint32_t band, uint32_t &r0, uint32_t &r1, uint32_t &s0,
                                                   uint32_t &s1) {
        r0 = band * j.rb;
        r1 = min(r0 + j.rb, j.out_h);
        const JP_GLOBAL int32_t *vb = tab + j.vb;
        s0 = (uint32_t)vb[2u * r0];
        s1 = (uint32_t)(vb[2u * (r1 - 1u)] + vb[2u * (r1 - 1u) + 1u]);
    }
    static __device__ __forceinline__ uint32_t chunks_of(const ResampleJob &j, const JP_GLOBAL int32_t *tab, uint32_t band) {
        uint32_t r0, r1, s0, s1;
        rows_of(j, tab, band, r0, r1, s0, s1);
        return (s1 - s0 + j.cap_rows - 1u) / j.cap_rows;
    }
    // the band's run of destination bytes [a, b) (offsets from dst) and its dwords [q0, q1)
    static __device__ __forceinline__ void run_of(const ResampleJob &j, uint32_t band, uint32_t &a, uint32_t &b, uint32_t &q0, uint32_t &q1) {
        const uint32_t rowb = j.out_w * j.nc, r0 = band * j.rb, r1 = min(r0 + j.rb, j.out_h);
        a = r0 * rowb, b = r1 * rowb;
        q0 = a >> 2, q1 = (b + 3u) >> 2;
    }
    // groups of RS_NT destination dwords in the band (the chunked path takes them one at a time)
    static __device__ __forceinline__ uint32_t groups_of(const ResampleJob &j, uint32_t band) {
        uint32_t a, b, q0, q1;
        run_of(j, band, a, b, q0, q1);
        return (q1 - q0 + RS_NT - 1u) / RS_NT;
    }
    // the output columns [x0, x1) whose horizontal pass group `group` of the band needs: a band of one row needs only the columns of
    // the group's own bytes (the chunked path repeats the pass per group), a taller one every column
    static __device__ __forceinline__ void group_columns(const ResampleJob &j, uint32_t band, uint32_t group, uint32_t &x0, uint32_t &x1) {
        x0 = 0u, x1 = j.out_w;
        if (j.rb != 1u) return;
        uint32_t a, b, q0, q1;
        run_of(j, band, a, b, q0, q1);
        const uint32_t f0 = max(4u * (q0 + group * RS_NT), a), f1 = min(4u * (q0 + (group + 1u) * RS_NT), b);
        if (f0 >= f1) return;
        x0 = (f0 - a) / j.nc, x1 = (f1 - a + j.nc - 1u) / j.nc;
    }

    // horizontal pass: columns [x0, x1) of the chunk's source rows [c0, c1) into LDS row (s - c0)
    static __device__ __forceinline__ void hpass(const ResampleJob &j, const JP_GLOBAL int32_t *tab, uint32_t band, uint32_t chunk, uint32_t x0, uint32_t x1,
                                                 uint32_t tid, uint8_t *lds) {
        uint32_t r0, r1, s0, s1;
        rows_of(j, tab, band, r0, r1, s0, s1);
        const uint32_t c0 = s0 + chunk * j.cap_rows, c1 = min(c0 + j.cap_rows, s1);
        if (c0 >= c1 || x0 >= x1) return;
        hpass_rows(j, tab, c0, c1 - c0, 0u, x0, x1, tid, lds);
    }
    // its core: columns [x0, x1) of the `nrows` source rows from c0 into the LDS rows from l0; nrows > 0 and x0 < x1 (the runs of
    // bands, DESIGN.md §4.15, pass only a band's new rows through it)
    static __device__ __forceinline__ void hpass_rows(const ResampleJob &j, const JP_GLOBAL int32_t *tab, uint32_t c0, uint32_t nrows, uint32_t l0, uint32_t x0,
                                                       uint32_t x1, uint32_t tid, uint8_t *lds) {
        const uint32_t nc = j.nc, nx = x1 - x0, units = ((nrows + RS_HROWS - 1u) / RS_HROWS) * nx;
        const size_t src_pitch = (size_t)j.in_w * nc;
        const JP_GLOBAL int32_t *hb = tab + j.hb;
        const JP_GLOBAL int32_t *hk = tab + j.hk;
        const JP_GLOBAL uint8_t *src = (const JP_GLOBAL uint8_t *)j.src;
#pragma unroll 1
        for (uint32_t u = tid; u < units; u += RS_NT) {
            const uint32_t rg = u / nx, xx = x0 + (u - rg * nx), row0 = rg * RS_HROWS;
            const uint32_t xmin = (uint32_t)hb[2u * xx], n = (uint32_t)hb[2u * xx + 1u];
            const JP_GLOBAL int32_t *k = hk + (size_t)xx * j.hks;
            // the span's bytes of every row as aligned dwords, whatever the row's alignment (a row beyond the chunk reads the chunk's last)
            const JP_GLOBAL uint32_t *pd[RS_HROWS];
            uint32_t cur[RS_HROWS], pos[RS_HROWS];
            int32_t sum[RS_HROWS][4];
#pragma unroll
            for (uint32_t i = 0; i < RS_HROWS; i++) {
                const uint32_t row = min(row0 + i, nrows - 1u);
                const JP_GLOBAL uint8_t *p = src + (size_t)(c0 + row) * src_pitch + (size_t)xmin * nc;
                const uint32_t m = (uint32_t)(uintptr_t)p & 3u;
                pd[i] = reinterpret_cast<const JP_GLOBAL uint32_t *>(p - m);
                pos[i] = m;
#pragma unroll
                for (uint32_t c = 0; c < 4; c++) sum[i][c] = 1 << (RS_PRECISION_BITS - 1);
            }
#pragma unroll
            for (uint32_t i = 0; i < RS_HROWS; i++) cur[i] = *pd[i];
            for (uint32_t x = 0; x < n; x++) {
                const int32_t kx = k[x];
#pragma unroll
                for (uint32_t c = 0; c < 4; c++)
                    if (c < nc) {
#pragma unroll
                        for (uint32_t i = 0; i < RS_HROWS; i++) {
                            if (pos[i] == 4u) {
                                pd[i]++;
                                cur[i] = *pd[i];
                                pos[i] = 0u;
                            }
                            sum[i][c] += (int32_t)((cur[i] >> (8u * pos[i])) & 255u) * kx;
                            pos[i]++;
                        }
                    }
            }
#pragma unroll
            for (uint32_t i = 0; i < RS_HROWS; i++) {
                if (row0 + i >= nrows) continue;
                uint8_t *o = lds + (l0 + row0 + i) * j.pitch + xx * nc;
#pragma unroll
                for (uint32_t c = 0; c < 4; c++)
                    if (c < nc) {
                        int32_t v = sum[i][c] >> RS_PRECISION_BITS;
                        v = v < 0 ? 0 : (v > 255 ? 255 : v);
                        o[c] = (uint8_t)v;
                    }
            }
        }
    }

    // ---- RGB output: convert, then resample.  The horizontal pass of a source of one or four channels that leaves
    // the three-channel u8 rows in LDS which hpass leaves for a three-channel source; everything behind it runs with nc = 3. ----
    // SNC = 1, R = G = B = v: replication commutes with the resample, so one sum per row, its rounded value written three times.
    // SNC = 3: the source as it is.  The byte walk of hpass (a gray window row starts at any byte) with the channels known.
    template <uint32_t SNC>
    static __device__ __forceinline__ void hpass_walk(const ResampleJob &j, const JP_GLOBAL int32_t *tab, uint32_t band, uint32_t chunk, uint32_t x0, uint32_t x1,
                                                      uint32_t tid, uint8_t *lds) {
        uint32_t r0, r1, s0, s1;
        rows_of(j, tab, band, r0, r1, s0, s1);
        const uint32_t c0 = s0 + chunk * j.cap_rows, c1 = min(c0 + j.cap_rows, s1);
        if (c0 >= c1 || x0 >= x1) return;
        hpass_walk_rows<SNC>(j, tab, c0, c1 - c0, 0u, x0, x1, tid, lds);
    }
    template <uint32_t SNC>
    static __device__ __forceinline__ void hpass_walk_rows(const ResampleJob &j, const JP_GLOBAL int32_t *tab, uint32_t c0, uint32_t nrows, uint32_t l0, uint32_t x0,
                                                            uint32_t x1, uint32_t tid, uint8_t *lds) {
        const uint32_t nx = x1 - x0, units = ((nrows + RS_HROWS - 1u) / RS_HROWS) * nx;
        const size_t src_pitch = (size_t)j.in_w * SNC;
        const JP_GLOBAL int32_t *hb = tab + j.hb;
        const JP_GLOBAL int32_t *hk = tab + j.hk;
        const JP_GLOBAL uint8_t *src = (const JP_GLOBAL uint8_t *)j.src;
#pragma unroll 1
        for (uint32_t u = tid; u < units; u += RS_NT) {
            const uint32_t rg = u / nx, xx = x0 + (u - rg * nx), row0 = rg * RS_HROWS;
            const uint32_t xmin = (uint32_t)hb[2u * xx], n = (uint32_t)hb[2u * xx + 1u];
            const JP_GLOBAL int32_t *k = hk + (size_t)xx * j.hks;
            const JP_GLOBAL uint32_t *pd[RS_HROWS];
            uint32_t cur[RS_HROWS], pos[RS_HROWS];
            int32_t sum[RS_HROWS][SNC];
#pragma unroll
            for (uint32_t i = 0; i < RS_HROWS; i++) {
                const uint32_t row = min(row0 + i, nrows - 1u);
                const JP_GLOBAL uint8_t *p = src + (size_t)(c0 + row) * src_pitch + (size_t)xmin * SNC;
                const uint32_t m = (uint32_t)(uintptr_t)p & 3u;
                pd[i] = reinterpret_cast<const JP_GLOBAL uint32_t *>(p - m);
                pos[i] = m;
#pragma unroll
                for (uint32_t c = 0; c < SNC; c++) sum[i][c] = 1 << (RS_PRECISION_BITS - 1);
            }
#pragma unroll
            for (uint32_t i = 0; i < RS_HROWS; i++) cur[i] = *pd[i];
#pragma clang loop vectorize(disable) interleave(disable)  // (taps two at a time cost more registers than the kernel has)
            for (uint32_t x = 0; x < n; x++) {
                const int32_t kx = k[x];
#pragma unroll
                for (uint32_t c = 0; c < SNC; c++) {
#pragma unroll
                    for (uint32_t i = 0; i < RS_HROWS; i++) {
                        if (pos[i] == 4u) {
                            pd[i]++;
                            cur[i] = *pd[i];
                            pos[i] = 0u;
                        }
                        sum[i][c] += (int32_t)((cur[i] >> (8u * pos[i])) & 255u) * kx;
                        pos[i]++;
                    }
                }
            }
#pragma unroll
            for (uint32_t i = 0; i < RS_HROWS; i++) {
                if (row0 + i >= nrows) continue;
                uint8_t *o = lds + (l0 + row0 + i) * j.pitch + xx * 3u;
#pragma unroll
                for (uint32_t c = 0; c < SNC; c++) {
                    int32_t v = sum[i][c] >> RS_PRECISION_BITS;
                    v = v < 0 ? 0 : (v > 255 ? 255 : v);
                    if (SNC == 1u) o[0] = o[1] = o[2] = (uint8_t)v;
                    else o[c] = (uint8_t)v;
                }
            }
        }
    }
    // Pillow's cmyk2rgb for one ink X under nk = 255 - K, in 32-bit integers: nk - round(X nk / 255); never outside 0..nk
    static __device__ __forceinline__ uint32_t cmyk_ink(uint32_t x, uint32_t nk) {
        const uint32_t t = x * nk + 128u;
        return nk - (((t >> 8) + t) >> 8);
    }
    // four channels (C, M, Y, K ink, 0 = none): a source pixel is one dword — window rows of w * 4 bytes behind a 256-byte aligned
    // image base are 4-aligned — converted BEFORE it is weighted (the conversion is not linear), three sums per row
    static __device__ __forceinline__ void hpass_cmyk(const ResampleJob &j, const JP_GLOBAL int32_t *tab, uint32_t band, uint32_t chunk, uint32_t x0, uint32_t x1,
                                                      uint32_t tid, uint8_t *lds) {
        uint32_t r0, r1, s0, s1;
        rows_of(j, tab, band, r0, r1, s0, s1);
        const uint32_t c0 = s0 + chunk * j.cap_rows, c1 = min(c0 + j.cap_rows, s1);
        if (c0 >= c1 || x0 >= x1) return;
        hpass_cmyk_rows(j, tab, c0, c1 - c0, 0u, x0, x1, tid, lds);
    }
    static __device__ __forceinline__ void hpass_cmyk_rows(const ResampleJob &j, const JP_GLOBAL int32_t *tab, uint32_t c0, uint32_t nrows, uint32_t l0, uint32_t x0,
                                                            uint32_t x1, uint32_t tid, uint8_t *lds) {
        const uint32_t nx = x1 - x0, units = ((nrows + RS_HROWS - 1u) / RS_HROWS) * nx;
        const JP_GLOBAL int32_t *hb = tab + j.hb;
        const JP_GLOBAL int32_t *hk = tab + j.hk;
        const JP_GLOBAL uint32_t *src = (const JP_GLOBAL uint32_t *)j.src;
#pragma unroll 1
        for (uint32_t u = tid; u < units; u += RS_NT) {
            const uint32_t rg = u / nx, xx = x0 + (u - rg * nx), row0 = rg * RS_HROWS;
            const uint32_t xmin = (uint32_t)hb[2u * xx], n = (uint32_t)hb[2u * xx + 1u];
            const JP_GLOBAL int32_t *k = hk + (size_t)xx * j.hks;
            const JP_GLOBAL uint32_t *pd[RS_HROWS];
            int32_t sum[RS_HROWS][3];
#pragma unroll
            for (uint32_t i = 0; i < RS_HROWS; i++) {  // (a row beyond the chunk reads the chunk's last)
                const uint32_t row = min(row0 + i, nrows - 1u);
                pd[i] = src + (size_t)(c0 + row) * j.in_w + xmin;
#pragma unroll
                for (uint32_t c = 0; c < 3; c++) sum[i][c] = 1 << (RS_PRECISION_BITS - 1);
            }
#pragma clang loop vectorize(disable) interleave(disable)  // (taps two at a time cost more registers than the kernel has)
            for (uint32_t x = 0; x < n; x++) {
                const int32_t kx = k[x];
#pragma unroll
                for (uint32_t i = 0; i < RS_HROWS; i++) {
                    const uint32_t d = pd[i][x], nk = 255u - (d >> 24);
#pragma unroll
                    for (uint32_t c = 0; c < 3; c++) sum[i][c] += (int32_t)cmyk_ink((d >> (8u * c)) & 255u, nk) * kx;
                }
            }
#pragma unroll
            for (uint32_t i = 0; i < RS_HROWS; i++) {
                if (row0 + i >= nrows) continue;
                uint8_t *o = lds + (l0 + row0 + i) * j.pitch + xx * 3u;
#pragma unroll
                for (uint32_t c = 0; c < 3; c++) {
                    int32_t v = sum[i][c] >> RS_PRECISION_BITS;
                    v = v < 0 ? 0 : (v > 255 ? 255 : v);
                    o[c] = (uint8_t)v;
                }
            }
        }
    }
    // the horizontal pass for a source of KIND channels that leaves three-channel rows (1: gray, 4: CMYK); 0: hpass
    template <uint32_t KIND>
    static __device__ __forceinline__ void hpass_of(const ResampleJob &j, const JP_GLOBAL int32_t *tab, uint32_t band, uint32_t chunk, uint32_t x0, uint32_t x1,
                                                    uint32_t tid, uint8_t *lds) {
        if (KIND == 1u) hpass_walk<1u>(j, tab, band, chunk, x0, x1, tid, lds);
        else if (KIND == 4u) hpass_cmyk(j, tab, band, chunk, x0, x1, tid, lds);
        else hpass(j, tab, band, chunk, x0, x1, tid, lds);
    }

    template <uint32_t KIND>
    static __device__ __forceinline__ void hpass_rows_of(const ResampleJob &j, const JP_GLOBAL int32_t *tab, uint32_t c0, uint32_t nrows, uint32_t l0, uint32_t tid,
                                                         uint8_t *lds) {
        if (KIND == 1u) hpass_walk_rows<1u>(j, tab, c0, nrows, l0, 0u, j.out_w, tid, lds);
        else if (KIND == 4u) hpass_cmyk_rows(j, tab, c0, nrows, l0, 0u, j.out_w, tid, lds);
        else hpass_rows(j, tab, c0, nrows, l0, 0u, j.out_w, tid, lds);
    }

    // ---- runs of bands: what band `band` (not the first of its run) keeps of the band before.  The rows [s0, p1) both read lie `shift`
    // rows too high in LDS (`keep` of them); its new rows are [n0, s1).  (xmin and xmin + n never decrease from one output row to the next.)
    static __device__ __forceinline__ void roll_of(const ResampleJob &j, const JP_GLOBAL int32_t *tab, uint32_t band, uint32_t &shift, uint32_t &keep, uint32_t &n0,
                                                   uint32_t &s0, uint32_t &s1) {
        uint32_t r0, r1, p0, p1;
        rows_of(j, tab, band - 1u, r0, r1, p0, p1);
        rows_of(j, tab, band, r0, r1, s0, s1);
        shift = s0 - p0;
        keep = p1 > s0 ? p1 - s0 : 0u;
        n0 = max(p1, s0);
    }
    // The move of the kept rows down by `shift` rows, slab by slab of RS_NT * RS_ROLL_DW dwords.  It goes toward lower addresses and
    // overlaps itself: a slab is READ into registers by every lane, then — behind a barrier — WRITTEN, and the next slab's reads wait
    // for another barrier.  (A slab's destination lies below its own source, so it never reaches a later slab's source.)
    static __device__ __forceinline__ uint32_t roll_slabs(const ResampleJob &j, uint32_t keep) {
        return (keep * (j.pitch >> 2) + RS_NT * RS_ROLL_DW - 1u) / (RS_NT * RS_ROLL_DW);
    }
    static __device__ __forceinline__ void roll_read(const ResampleJob &j, uint32_t shift, uint32_t keep, uint32_t slab, uint32_t tid, const uint8_t *lds,
                                                     uint32_t (&reg)[RS_ROLL_DW]) {
        const uint32_t total = keep * (j.pitch >> 2), off = shift * (j.pitch >> 2);
        const uint32_t *w = reinterpret_cast<const uint32_t *>(lds);
#pragma unroll
        for (uint32_t k = 0; k < RS_ROLL_DW; k++) {
            const uint32_t d = (slab * RS_ROLL_DW + k) * RS_NT + tid;
            reg[k] = d < total ? w[d + off] : 0u;
        }
    }
    static __device__ __forceinline__ void roll_write(const ResampleJob &j, uint32_t keep, uint32_t slab, uint32_t tid, uint8_t *lds, const uint32_t (&reg)[RS_ROLL_DW]) {
        const uint32_t total = keep * (j.pitch >> 2);
        uint32_t *w = reinterpret_cast<uint32_t *>(lds);
#pragma unroll
        for (uint32_t k = 0; k < RS_ROLL_DW; k++) {
            const uint32_t d = (slab * RS_ROLL_DW + k) * RS_NT + tid;
            if (d < total) w[d] = reg[k];
        }
    }

    // the share of source rows [c0, c1) (in LDS) in the four sums of destination dword q: where its bytes lie in one output row at a
    // multiple of four an aligned LDS dword per tap, else byte by byte
    static __device__ __forceinline__ void item_sum(const ResampleJob &j, const JP_GLOBAL int32_t *tab, uint32_t q, uint32_t a, uint32_t b, uint32_t c0,
                                                    uint32_t c1, const uint8_t *lds, int32_t (&sum)[4]) {
        const uint32_t rowb = j.out_w * j.nc;
        const JP_GLOBAL int32_t *vb = tab + j.vb;
        const JP_GLOBAL int32_t *vk = tab + j.vk;
        const uint32_t f0 = max(4u * q, a), f1 = min(4u * q + 4u, b);  // the dword's bytes inside the band
        const uint32_t row0 = f0 / rowb, col0 = f0 - row0 * rowb;
        if (f1 - f0 == 4u && col0 + 4u <= rowb && (col0 & 3u) == 0u) {
            const uint32_t ymin = (uint32_t)vb[2u * row0], n = (uint32_t)vb[2u * row0 + 1u];
            const uint32_t t0 = c0 > ymin ? c0 - ymin : 0u, t1 = min(n, c1 > ymin ? c1 - ymin : 0u);
            const JP_GLOBAL int32_t *k = vk + (size_t)row0 * j.vks;
            for (uint32_t t = t0; t < t1; t++) {
                const uint32_t d = *reinterpret_cast<const uint32_t *>(lds + (ymin + t - c0) * j.pitch + col0);
                const int32_t kt = k[t];
                sum[0] += (int32_t)(d & 255u) * kt;
                sum[1] += (int32_t)((d >> 8) & 255u) * kt;
                sum[2] += (int32_t)((d >> 16) & 255u) * kt;
                sum[3] += (int32_t)(d >> 24) * kt;
            }
            return;
        }
#pragma unroll
        for (uint32_t e = 0; e < 4; e++) {
            const uint32_t f = 4u * q + e;
            if (f < f0 || f >= f1) continue;
            const uint32_t row = f / rowb, col = f - row * rowb;
            const uint32_t ymin = (uint32_t)vb[2u * row], n = (uint32_t)vb[2u * row + 1u];
            const uint32_t t0 = c0 > ymin ? c0 - ymin : 0u, t1 = min(n, c1 > ymin ? c1 - ymin : 0u);
            const JP_GLOBAL int32_t *k = vk + (size_t)row * j.vks;
            int32_t s = 0;
            for (uint32_t t = t0; t < t1; t++) s += (int32_t)lds[(ymin + t - c0) * j.pitch + col] * k[t];
            sum[e] += s;
        }
    }
    // the sums rounded, clamped and stored: a whole dword where all four bytes are the band's, else its own bytes one by one (the
    // first / last dword of a band may be shared with its neighbour)
    static __device__ __forceinline__ void item_store(const ResampleJob &j, uint32_t q, uint32_t a, uint32_t b, const int32_t (&sum)[4]) {
        JP_GLOBAL uint8_t *dst = (JP_GLOBAL uint8_t *)j.dst;
        uint32_t v[4];
#pragma unroll
        for (uint32_t e = 0; e < 4; e++) {
            const int32_t s = (sum[e] + (1 << (RS_PRECISION_BITS - 1))) >> RS_PRECISION_BITS;
            v[e] = (uint32_t)(s < 0 ? 0 : (s > 255 ? 255 : s));
        }
        if (4u * q >= a && 4u * q + 4u <= b) {
            reinterpret_cast<JP_GLOBAL uint32_t *>(dst)[q] = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        } else {
#pragma unroll
            for (uint32_t e = 0; e < 4; e++)
                if (4u * q + e >= a && 4u * q + e < b) dst[4u * q + e] = (uint8_t)v[e];
        }
    }

    // vertical pass of a band whose source rows are one chunk: every destination dword summed and stored
    static __device__ __forceinline__ void vstore(const ResampleJob &j, const JP_GLOBAL int32_t *tab, uint32_t band, uint32_t tid, const uint8_t *lds) {
        uint32_t r0, r1, s0, s1, a, b, q0, q1;
        rows_of(j, tab, band, r0, r1, s0, s1);
        run_of(j, band, a, b, q0, q1);
#pragma unroll 1
        for (uint32_t q = q0 + tid; q < q1; q += RS_NT) {
            int32_t sum[4] = {0, 0, 0, 0};
            item_sum(j, tab, q, a, b, s0, s1, lds, sum);
            item_store(j, q, a, b, sum);
        }
    }
    // the chunked path: dword `tid` of group `group` gathers its sums (exact in int32) chunk by chunk in registers, then stores
    static __device__ __forceinline__ void vacc(const ResampleJob &j, const JP_GLOBAL int32_t *tab, uint32_t band, uint32_t chunk, uint32_t group, uint32_t tid,
                                                const uint8_t *lds, int32_t (&sum)[4]) {
        uint32_t r0, r1, s0, s1, a, b, q0, q1;
        rows_of(j, tab, band, r0, r1, s0, s1);
        run_of(j, band, a, b, q0, q1);
        const uint32_t c0 = s0 + chunk * j.cap_rows, c1 = min(c0 + j.cap_rows, s1), q = q0 + group * RS_NT + tid;
        if (q < q1 && c0 < c1) item_sum(j, tab, q, a, b, c0, c1, lds, sum);
    }
    static __device__ __forceinline__ void vput(const ResampleJob &j, uint32_t band, uint32_t group, uint32_t tid, const int32_t (&sum)[4]) {
        uint32_t a, b, q0, q1;
        run_of(j, band, a, b, q0, q1);
        const uint32_t q = q0 + group * RS_NT + tid;
        if (q < q1) item_store(j, q, a, b, sum);
    }
};

#endif  // JPGPU_RS_DEVICE_BODY

}  // namespace jpgpu

#if defined(__HIP__) && !defined(JPGPU_HOST_EMULATION)
#include <hip/hip_runtime.h>
namespace jpgpu {
// resample.hip: n_images jobs, their tables from d_tab; max_bands / lds_bytes over the jobs
// (rgb: the instance whose horizontal pass converts jobs with src_nc != 0 — a batch created with JPGPU_BATCH_RGB_OUTPUT)
hipError_t launch_resample_band(const ResampleJob *d_jobs, const int32_t *d_tab, uint32_t n_images, uint32_t max_bands, uint32_t lds_bytes, hipStream_t stream,
                                bool rgb = false);
// runs of bands: image i takes d_bpr[i] consecutive bands per workgroup (0: not in this launch); max_runs over the images
hipError_t launch_resample_run(const ResampleJob *d_jobs, const int32_t *d_tab, const uint32_t *d_bpr, uint32_t n_images, uint32_t max_runs, uint32_t lds_bytes,
                               hipStream_t stream);
}  // namespace jpgpu
#endif
