// tensor_band.hpp — the resample of resample_band.hpp with a tensor behind it (jpgpu_batch_create_tensor): every image
// of the batch resampled to one output size and written as nc planes of out_h x out_w elements (CHW, packed) of f32, f16 or bf16,
//     elem(c, r, x) = T[c][ u8(r, flip ? out_w - 1 - x : x, c) ]
// where u8 is what resample_band_kernel writes and T a table of nc x 256 elements made on the host (tensor_table below,
// = jpgpu_tensor_table).  The device looks T up and does no float arithmetic.
//
// The planner, the bands, the chunks and the horizontal pass (RBand::hpass, u8 rows in LDS) are resample_band.hpp's, unchanged.  New
// here: the vertical pass and the store, which write the tensor — there is no resized u8 image anywhere.
//   * out_w and the plane pitch multiples of four (every model's input size): an item is four pixels x all channels of one output
//     row — 4 nc contiguous LDS bytes per tap read as whole dwords, 4 nc sums, one 16-byte (f32) or 8-byte store per plane.
//   * else: an item is four consecutive elements of the flat tensor (an aligned 16 / 8 bytes, the image's base is 256-byte aligned),
//     summed from LDS bytes; an item the band shares with its neighbour, with the next plane or with the end of the row goes
//     element by element, and a band stores its own elements only.
//   * a flip mirrors the column READ from LDS; the stores stay where they are.
//   * T sits in LDS behind the rows (at most 4 kB: 32 + 4 kB per workgroup, four workgroups per CU).
//   * RGB output (JPGPU_BATCH_RGB_OUTPUT): nothing here knows of it — a gray or CMYK job arrives with nc = 3, its rows in
//     LDS are three-channel (RBand::hpass_of) and T is the table of three channels.
#pragma once
#include <string.h>

#include "resample_band.hpp"

namespace jpgpu {

constexpr uint32_t TN_F32 = 1, TN_F16 = 2, TN_BF16 = 3;  // JPGPU_TENSOR_*
constexpr uint32_t TN_TABLE_MAX = 4u * 256u * 4u;        // bytes of the largest table

inline uint32_t tensor_elem_bytes(uint32_t dtype) { return dtype == TN_F32 ? 4u : ((dtype == TN_F16 || dtype == TN_BF16) ? 2u : 0u); }

inline uint32_t tensor_f32_bits(float f) {
    uint32_t x;
    memcpy(&x, &f, 4);
    return x;
}
inline bool tensor_finite(float f) { return (tensor_f32_bits(f) & 0x7f800000u) != 0x7f800000u; }
// IEEE single -> binary16, round to nearest even
inline uint16_t tensor_f16_bits(float f) {
    uint32_t x = tensor_f32_bits(f);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
    const uint32_t e = x >> 23;
    if (e >= 143u) return (uint16_t)(sign | 0x7c00u);  // 2^16 and above (infinity included)
    if (e >= 113u) {                                    // normal (a carry out of the mantissa goes into the exponent, up to infinity)
        const uint32_t m = x & 0x7fffffu, rem = m & 0x1fffu;
        uint32_t h = ((e - 112u) << 10) | (m >> 13);
        if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) h++;
        return (uint16_t)(sign | h);
    }
    if (e >= 102u) {  // subnormal: units of 2^-24
        const uint32_t m = (x & 0x7fffffu) | 0x800000u, shift = 126u - e, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
        uint32_t h = m >> shift;
        if (rem > half || (rem == half && (h & 1u))) h++;
        return (uint16_t)(sign | h);
    }
    return (uint16_t)sign;
}
// IEEE single -> bfloat16, round to nearest even
inline uint16_t tensor_bf16_bits(float f) {
    uint32_t x = tensor_f32_bits(f);
    if ((x & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((x >> 16) | 0x40u);
    x += 0x7fffu + ((x >> 16) & 1u);
    return (uint16_t)(x >> 16);
}

// What a tensor format must be for images of up to `nc` channels: a known dtype, finite means, finite non-zero stds.
inline bool tensor_format_ok(uint32_t dtype, uint32_t reserved, const float *mean, const float *std_, uint32_t nc, const char *&why) {
    if (tensor_elem_bytes(dtype) == 0) return why = "unknown dtype", false;
    if (reserved != 0) return why = "reserved must be 0", false;
    if (nc == 0 || nc > 4) return why = "1..4 channels", false;
    for (uint32_t c = 0; c < nc; c++) {
        if (!tensor_finite(mean[c])) return why = "a mean is not finite", false;
        if (!tensor_finite(std_[c]) || std_[c] == 0.0f) return why = "a std is zero or not finite", false;
    }
    return true;
}
// T[c][v] for c < nc, v < 256: IEEE single, one operation per statement (nothing for a compiler to contract), then rounded once
inline void tensor_table(uint32_t dtype, const float *mean, const float *std_, uint32_t nc, void *table) {
    for (uint32_t c = 0; c < nc; c++)
        for (uint32_t v = 0; v < 256u; v++) {
            const float a = (float)v / 255.0f;
            const float b = a - mean[c];
            const float tt = b / std_[c];
            const size_t i = (size_t)c * 256u + v;
            if (dtype == TN_F32) ((uint32_t *)table)[i] = tensor_f32_bits(tt);
            else ((uint16_t *)table)[i] = dtype == TN_F16 ? tensor_f16_bits(tt) : tensor_bf16_bits(tt);
        }
}

// One image of the launch: the resample's job (dst: the image's tensor, 256-byte aligned), the pitch of a plane and the flip.
struct TensorJob {
    ResampleJob r;
    uint32_t plane;  // elements from one plane to the next (the batch: out_h * out_w)
    uint32_t flip;   // != 0: columns mirrored
};

#ifdef JPGPU_RS_DEVICE_BODY
// E: the element as its bits (uint32_t for f32, uint16_t for f16 / bf16)
template <class E>
struct TBand {
    static constexpr uint32_t ES = (uint32_t)sizeof(E);

    static __device__ __forceinline__ bool fast(const TensorJob &t) { return ((t.r.out_w | t.plane) & 3u) == 0u; }
    static __device__ __forceinline__ uint32_t table_offset(const ResampleJob &j) { return (j.lds_bytes + 15u) & ~15u; }
    static __device__ __forceinline__ const E *table_of(const ResampleJob &j, const uint8_t *lds) { return reinterpret_cast<const E *>(lds + table_offset(j)); }
    // the table into LDS, behind the rows
    static __device__ __forceinline__ void load_table(const TensorJob &t, const JP_GLOBAL uint32_t *ttab, uint32_t tid, uint8_t *lds) {
        uint32_t *T = reinterpret_cast<uint32_t *>(lds + table_offset(t.r));
        const uint32_t words = t.r.nc * 256u * ES / 4u;
        for (uint32_t w = tid; w < words; w += RS_NT) T[w] = ttab[w];
    }

    static __device__ __forceinline__ uint32_t round_u8(int32_t s) {
        s = (s + (1 << (RS_PRECISION_BITS - 1))) >> RS_PRECISION_BITS;
        return (uint32_t)(s < 0 ? 0 : (s > 255 ? 255 : s));
    }
    // four elements at an aligned 4 * ES bytes
    static __device__ __forceinline__ void store4(JP_GLOBAL uint8_t *p, const E (&e)[4]) {
        if (ES == 4u) {
            const v4u v = {(uint32_t)e[0], (uint32_t)e[1], (uint32_t)e[2], (uint32_t)e[3]};
            *reinterpret_cast<JP_GLOBAL v4u *>(p) = v;
        } else {
            const v2u v = {(uint32_t)e[0] | ((uint32_t)e[1] << 16), (uint32_t)e[2] | ((uint32_t)e[3] << 16)};
            *reinterpret_cast<JP_GLOBAL v2u *>(p) = v;
        }
    }
    // the taps [t0, t1) of output row `row` that lie in the source rows [c0, c1)
    static __device__ __forceinline__ void taps_of(const ResampleJob &j, const JP_GLOBAL int32_t *tab, uint32_t row, uint32_t c0, uint32_t c1, uint32_t &ymin,
                                                   uint32_t &t0, uint32_t &t1) {
        const JP_GLOBAL int32_t *vb = tab + j.vb;
        ymin = (uint32_t)vb[2u * row];
        const uint32_t n = (uint32_t)vb[2u * row + 1u];
        t0 = c0 > ymin ? c0 - ymin : 0u, t1 = min(n, c1 > ymin ? c1 - ymin : 0u);
    }

    // ---- out_w and the plane pitch multiples of four: items of four pixels x NC channels ----
    // item w of the band: row r, columns [x, x + 4)
    static __device__ __forceinline__ void fast_item(const ResampleJob &j, uint32_t band, uint32_t w, uint32_t &r, uint32_t &x) {
        const uint32_t xq = j.out_w >> 2, rr = w / xq;
        r = band * j.rb + rr, x = 4u * (w - rr * xq);
    }
    // the share of source rows [c0, c1) in the item's 4 NC sums, in the order of the LDS bytes read (pixel-major; mirrored with a flip)
    template <uint32_t NC>
    static __device__ __forceinline__ void fast_sum(const TensorJob &t, const JP_GLOBAL int32_t *tab, uint32_t r, uint32_t x, uint32_t c0, uint32_t c1,
                                                    const uint8_t *lds, int32_t (&sum)[16]) {
        const ResampleJob &j = t.r;
        uint32_t ymin, t0, t1;
        taps_of(j, tab, r, c0, c1, ymin, t0, t1);
        const JP_GLOBAL int32_t *k = tab + j.vk + (size_t)r * j.vks;
        const uint32_t xs = t.flip ? j.out_w - 4u - x : x;
        const uint8_t *p = lds + xs * NC;  // (4 NC bytes at a multiple of 4 NC: the pitch is out_w * NC)
        for (uint32_t tt = t0; tt < t1; tt++) {
            const uint8_t *q = p + (ymin + tt - c0) * j.pitch;
            const int32_t kt = k[tt];
            uint32_t w[4] = {0, 0, 0, 0};
            if (NC == 4u) {
                const v4u v = *reinterpret_cast<const v4u *>(q);
                w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
            } else if (NC == 2u) {
                const v2u v = *reinterpret_cast<const v2u *>(q);
                w[0] = v.x, w[1] = v.y;
            } else {
#pragma unroll
                for (uint32_t i = 0; i < NC; i++) w[i] = reinterpret_cast<const uint32_t *>(q)[i];
            }
#pragma unroll
            for (uint32_t b = 0; b < 4u * NC; b++) sum[b] += (int32_t)((w[b >> 2] >> (8u * (b & 3u))) & 255u) * kt;
        }
    }
    template <uint32_t NC>
    static __device__ __forceinline__ void fast_store(const TensorJob &t, uint32_t r, uint32_t x, const int32_t (&sum)[16], const uint8_t *lds) {
        const ResampleJob &j = t.r;
        const E *T = table_of(j, lds);
        JP_GLOBAL uint8_t *dst = (JP_GLOBAL uint8_t *)j.dst;
#pragma unroll
        for (uint32_t c = 0; c < NC; c++) {
            E e[4];
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) e[i] = T[c * 256u + round_u8(t.flip ? sum[(3u - i) * NC + c] : sum[i * NC + c])];
            store4(dst + ((size_t)c * t.plane + (size_t)r * j.out_w + x) * ES, e);
        }
    }

    // ---- any size: items of four consecutive elements of the flat tensor ----
    // plane c's elements of the band [a, b) and their items [q0, q1)
    static __device__ __forceinline__ void run_of(const TensorJob &t, uint32_t band, uint32_t c, uint32_t &a, uint32_t &b, uint32_t &q0, uint32_t &q1) {
        const ResampleJob &j = t.r;
        const uint32_t r0 = band * j.rb, r1 = min(r0 + j.rb, j.out_h);
        a = c * t.plane + r0 * j.out_w, b = c * t.plane + r1 * j.out_w;
        q0 = a >> 2, q1 = (b + 3u) >> 2;
    }
    // item w of the band -> its plane and item; false beyond the band's items
    static __device__ __forceinline__ bool item_of(const TensorJob &t, uint32_t band, uint32_t w, uint32_t &c, uint32_t &q, uint32_t &a, uint32_t &b) {
        for (c = 0; c < t.r.nc; c++) {
            uint32_t q0, q1;
            run_of(t, band, c, a, b, q0, q1);
            if (w < q1 - q0) return q = q0 + w, true;
            w -= q1 - q0;
        }
        return false;
    }
    // the share of source rows [c0, c1) in the sums of item q's elements of plane c: one walk over the taps where all four lie in one
    // row, else element by element
    static __device__ __forceinline__ void item_sum(const TensorJob &t, const JP_GLOBAL int32_t *tab, uint32_t c, uint32_t q, uint32_t a, uint32_t b, uint32_t c0,
                                                    uint32_t c1, const uint8_t *lds, int32_t (&sum)[16]) {
        const ResampleJob &j = t.r;
        const uint32_t nc = j.nc, ow = j.out_w, base = c * t.plane;
        const uint32_t f0 = max(4u * q, a), f1 = min(4u * q + 4u, b);  // the item's elements inside the band's run
        const JP_GLOBAL int32_t *vk = tab + j.vk;
        const uint32_t row0 = (f0 - base) / ow, x0 = (f0 - base) - row0 * ow;
        if (f1 - f0 == 4u && x0 + 4u <= ow) {
            uint32_t ymin, t0, t1;
            taps_of(j, tab, row0, c0, c1, ymin, t0, t1);
            const JP_GLOBAL int32_t *k = vk + (size_t)row0 * j.vks;
            const uint32_t col = (t.flip ? ow - 1u - x0 : x0) * nc + c;
            const int32_t step = t.flip ? -(int32_t)nc : (int32_t)nc;
            for (uint32_t tt = t0; tt < t1; tt++) {
                const uint8_t *p = lds + (ymin + tt - c0) * j.pitch + col;
                const int32_t kt = k[tt];
#pragma unroll
                for (int32_t e = 0; e < 4; e++) sum[e] += (int32_t)p[e * step] * kt;
            }
            return;
        }
#pragma unroll
        for (uint32_t e = 0; e < 4; e++) {
            const uint32_t f = 4u * q + e;
            if (f < f0 || f >= f1) continue;
            const uint32_t row = (f - base) / ow, x = (f - base) - row * ow;
            uint32_t ymin, t0, t1;
            taps_of(j, tab, row, c0, c1, ymin, t0, t1);
            const JP_GLOBAL int32_t *k = vk + (size_t)row * j.vks;
            const uint32_t col = (t.flip ? ow - 1u - x : x) * nc + c;
            int32_t s = 0;
            for (uint32_t tt = t0; tt < t1; tt++) s += (int32_t)lds[(ymin + tt - c0) * j.pitch + col] * k[tt];
            sum[e] += s;
        }
    }
    // rounded, looked up and stored: one wide store where all four elements are the band's, else its own one by one
    static __device__ __forceinline__ void item_store(const TensorJob &t, uint32_t c, uint32_t q, uint32_t a, uint32_t b, const int32_t (&sum)[16],
                                                      const uint8_t *lds) {
        const E *T = table_of(t.r, lds) + c * 256u;
        JP_GLOBAL uint8_t *dst = (JP_GLOBAL uint8_t *)t.r.dst;
        E e[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) e[i] = T[round_u8(sum[i])];
        if (4u * q >= a && 4u * q + 4u <= b) {
            store4(dst + (size_t)q * 4u * ES, e);
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 4; i++)
                if (4u * q + i >= a && 4u * q + i < b) reinterpret_cast<JP_GLOBAL E *>(dst)[4u * q + i] = e[i];
        }
    }

    // ---- the band ----
    static __device__ __forceinline__ uint32_t items_of(const TensorJob &t, uint32_t band) {
        const ResampleJob &j = t.r;
        const uint32_t r0 = band * j.rb, r1 = min(r0 + j.rb, j.out_h);
        if (fast(t)) return (r1 - r0) * (j.out_w >> 2);
        uint32_t n = 0;
        for (uint32_t c = 0; c < j.nc; c++) {
            uint32_t a, b, q0, q1;
            run_of(t, band, c, a, b, q0, q1);
            n += q1 - q0;
        }
        return n;
    }
    // groups of RS_NT items (the chunked path takes them one at a time)
    static __device__ __forceinline__ uint32_t groups_of(const TensorJob &t, uint32_t band) { return (items_of(t, band) + RS_NT - 1u) / RS_NT; }
    // the output columns [x0, x1) whose horizontal pass group `group` needs: a band of one row with four-pixel items only its own
    // columns (mirrored with a flip), any other every column
    static __device__ __forceinline__ void group_columns(const TensorJob &t, uint32_t band, uint32_t group, uint32_t &x0, uint32_t &x1) {
        const ResampleJob &j = t.r;
        x0 = 0u, x1 = j.out_w;
        if (j.rb != 1u || !fast(t)) return;
        const uint32_t i0 = group * RS_NT, i1 = min(i0 + RS_NT, j.out_w >> 2);
        if (i0 >= i1) return;
        x0 = t.flip ? j.out_w - 4u * i1 : 4u * i0, x1 = t.flip ? j.out_w - 4u * i0 : 4u * i1;
    }
    // the share of source rows [c0, c1) in item w of the band
    static __device__ __forceinline__ void sum_item(const TensorJob &t, const JP_GLOBAL int32_t *tab, uint32_t band, uint32_t w, uint32_t c0, uint32_t c1,
                                                    const uint8_t *lds, int32_t (&sum)[16]) {
        if (fast(t)) {
            uint32_t r, x;
            fast_item(t.r, band, w, r, x);
            switch (t.r.nc) {  // (uniform)
            case 1: fast_sum<1>(t, tab, r, x, c0, c1, lds, sum); break;
            case 2: fast_sum<2>(t, tab, r, x, c0, c1, lds, sum); break;
            case 3: fast_sum<3>(t, tab, r, x, c0, c1, lds, sum); break;
            default: fast_sum<4>(t, tab, r, x, c0, c1, lds, sum); break;
            }
            return;
        }
        uint32_t c, q, a, b;
        if (item_of(t, band, w, c, q, a, b)) item_sum(t, tab, c, q, a, b, c0, c1, lds, sum);
    }
    static __device__ __forceinline__ void store_item(const TensorJob &t, uint32_t band, uint32_t w, const int32_t (&sum)[16], const uint8_t *lds) {
        if (fast(t)) {
            uint32_t r, x;
            fast_item(t.r, band, w, r, x);
            switch (t.r.nc) {
            case 1: fast_store<1>(t, r, x, sum, lds); break;
            case 2: fast_store<2>(t, r, x, sum, lds); break;
            case 3: fast_store<3>(t, r, x, sum, lds); break;
            default: fast_store<4>(t, r, x, sum, lds); break;
            }
            return;
        }
        uint32_t c, q, a, b;
        if (item_of(t, band, w, c, q, a, b)) item_store(t, c, q, a, b, sum, lds);
    }

    // vertical pass of a band whose source rows are one chunk: every item summed and stored
    static __device__ __forceinline__ void vstore(const TensorJob &t, const JP_GLOBAL int32_t *tab, uint32_t band, uint32_t tid, const uint8_t *lds) {
        uint32_t r0, r1, s0, s1;
        RBand::rows_of(t.r, tab, band, r0, r1, s0, s1);
        const uint32_t items = items_of(t, band);
#pragma unroll 1
        for (uint32_t w = tid; w < items; w += RS_NT) {
            int32_t sum[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            sum_item(t, tab, band, w, s0, s1, lds, sum);
            store_item(t, band, w, sum, lds);
        }
    }
    // the chunked path: item `tid` of group `group` gathers its sums (exact in int32) chunk by chunk in registers, then stores
    static __device__ __forceinline__ void vacc(const TensorJob &t, const JP_GLOBAL int32_t *tab, uint32_t band, uint32_t chunk, uint32_t group, uint32_t tid,
                                                const uint8_t *lds, int32_t (&sum)[16]) {
        uint32_t r0, r1, s0, s1;
        RBand::rows_of(t.r, tab, band, r0, r1, s0, s1);
        const uint32_t c0 = s0 + chunk * t.r.cap_rows, c1 = min(c0 + t.r.cap_rows, s1), w = group * RS_NT + tid;
        if (w < items_of(t, band) && c0 < c1) sum_item(t, tab, band, w, c0, c1, lds, sum);
    }
    static __device__ __forceinline__ void vput(const TensorJob &t, uint32_t band, uint32_t group, uint32_t tid, const int32_t (&sum)[16], const uint8_t *lds) {
        const uint32_t w = group * RS_NT + tid;
        if (w < items_of(t, band)) store_item(t, band, w, sum, lds);
    }
};
#endif  // JPGPU_RS_DEVICE_BODY

}  // namespace jpgpu

#if defined(__HIP__) && !defined(JPGPU_HOST_EMULATION)
namespace jpgpu {
// resample.hip: n_images jobs, their resample tables from d_tab, the tensor table (4 x 256 elements of elem_bytes) from d_ttab;
// max_bands / lds_bytes (the rows') over the jobs; rgb: the instances whose horizontal pass converts jobs with src_nc != 0
hipError_t launch_resample_tensor(const TensorJob *d_jobs, const int32_t *d_tab, const void *d_ttab, uint32_t elem_bytes, uint32_t n_images, uint32_t max_bands,
                                  uint32_t lds_bytes, hipStream_t stream, bool rgb = false);
// runs of bands (resample_band.hpp): image i takes d_bpr[i] consecutive bands per workgroup (0: not in this launch)
hipError_t launch_resample_tensor_run(const TensorJob *d_jobs, const int32_t *d_tab, const void *d_ttab, const uint32_t *d_bpr, uint32_t elem_bytes, uint32_t n_images,
                                      uint32_t max_runs, uint32_t lds_bytes, hipStream_t stream);
}  // namespace jpgpu
#endif
