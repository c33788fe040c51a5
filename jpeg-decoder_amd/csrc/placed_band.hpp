// placed_band.hpp — the resample of resample_band.hpp / tensor_band.hpp with a placement (jpgpu_batch_create_placed):
// every image's source is resampled to a size of its own, rw x rh, and laid at (x, y) into the batch's out_w x out_h canvas; what falls
// outside is cropped, what the image does not cover is `fill`.
//
// Every output pixel of the two-pass resample depends on its own row and column of the tables only, so the visible part of the
// rw x rh resample IS a resample job of its own: out_w x out_h = the visible columns x rows, its tables the entries
// [first, first + count) of the axes' tables (resample_coefficients_range).  Nothing outside the visible part is computed.
//
//   1. planner (placed_plan, no HIP dependency): the inner ResampleJob is planned over the visible rows as resample_plan plans a whole
//      image — rb, cap_rows, bands — so padding does not shrink the bands.  The canvas rows are cut into bands of rb rows whose
//      boundaries coincide with the inner bands': `pre` bands above the first visible row, then the inner bands (the last one takes the
//      filled rows below it up to its rb), then bands of fill.  A band without a visible row touches neither the source nor LDS rows.
//   2. horizontal pass: RBand::hpass / hpass_of of the inner job, unchanged — visible columns only, LDS rows of visible width.  The rows
//      begin `shift` = (vx * nc) & 15 bytes into LDS and their pitch is a multiple of 16, so that a visible byte's LDS address is
//      congruent to its canvas column's byte modulo 16: a destination dword whose bytes are all visible is an aligned LDS dword whenever
//      the canvas row is a multiple of four bytes, and the tensor's four-pixel items read whole aligned dwords as TBand's do.
//   3. vertical pass and store (PBand): one lane per destination dword of the canvas.  A dword whose four bytes are visible in one row
//      takes aligned LDS dwords; any other goes byte by byte: a visible byte is summed, a filled byte IS the fill (never weighted).  A
//      band stores its own bytes only.
//   4. tensor (PTBand): the items of tensor_band.hpp over the canvas; the flip mirrors the canvas column before the visible / filled
//      decision, a filled element is T[c][fill[c]].
#pragma once
#include <math.h>

#include "tensor_band.hpp"

namespace jpgpu {

// Entries [first, first + count) of the tables resample_coefficients(in_size, out_size, ...) gives: bounds[2 i], bounds[2 i + 1] and
// coefs[i * ksize + x] belong to output index first + i.  The statements are resample_coefficients', entry by entry.
inline void resample_coefficients_range(uint32_t in_size, uint32_t out_size, uint32_t first, uint32_t count, int32_t *bounds, int32_t *coefs, uint32_t ksize) {
    resample_coefficients_range_filtered(RS_FILTER_BILINEAR, in_size, out_size, first, count, bounds, coefs, ksize);
}

// The visible range of one axis: a resample of `r` entries laid at `at` in a canvas of `out`.  False when nothing shows.
inline bool placed_axis(uint32_t r, int32_t at, uint32_t out, uint32_t &first, uint32_t &count, uint32_t &v0) {
    const int64_t lo = at < 0 ? 0 : (int64_t)at, hi = (int64_t)at + (int64_t)r < (int64_t)out ? (int64_t)at + (int64_t)r : (int64_t)out;
    if (r == 0 || lo >= hi) return false;
    first = (uint32_t)(lo - (int64_t)at), count = (uint32_t)(hi - lo), v0 = (uint32_t)lo;
    return true;
}

// The placement rules of jpgpu_fit_placement (include/jpgpu.h; modes 0 stretch, 1 shorter side + centre crop, 2 letterbox).  False for
// what the rule refuses.
inline bool fit_placement(uint32_t mode, uint32_t size, uint32_t src_w, uint32_t src_h, uint32_t out_w, uint32_t out_h, uint32_t &rw, uint32_t &rh, int32_t &x,
                          int32_t &y) {
    if (src_w == 0 || src_h == 0 || out_w == 0 || out_h == 0 || out_w > 65535u || out_h > 65535u) return false;
    if (mode == 0u) return rw = out_w, rh = out_h, x = y = 0, true;
    if (mode == 1u) {  // torchvision's Resize(size) then CenterCrop((out_h, out_w))
        if (size == 0u) return false;
        uint64_t w, h;
        if (src_w <= src_h) w = size, h = (uint64_t)size * src_h / src_w;
        else h = size, w = (uint64_t)size * src_w / src_h;
        if (w == 0 || h == 0 || w > 65535u || h > 65535u) return false;
        rw = (uint32_t)w, rh = (uint32_t)h;
        auto offset = [](int64_t r, int64_t out) -> int32_t {
            const int64_t d = r - out;
            if (d < 0) return (int32_t)((-d) / 2);  // center_crop pads (out - r) // 2 on the left / top
            int64_t half = d / 2;                  // round(d / 2.0): a half goes to the even neighbour
            if ((d & 1) && (half & 1)) half++;
            return (int32_t)-half;
        };
        x = offset((int64_t)rw, (int64_t)out_w), y = offset((int64_t)rh, (int64_t)out_h);
        return true;
    }
    if (mode == 2u) {  // letterbox: IEEE double, one operation per statement
        const double rx = (double)out_w / (double)src_w;
        const double ry = (double)out_h / (double)src_h;
        const double r = rx < ry ? rx : ry;
        const double fw = (double)src_w * r;
        const double fh = (double)src_h * r;
        double w = rint(fw), h = rint(fh);
        if (w < 1.0) w = 1.0;
        if (h < 1.0) h = 1.0;
        if (w > (double)out_w) w = (double)out_w;
        if (h > (double)out_h) h = (double)out_h;
        rw = (uint32_t)w, rh = (uint32_t)h;
        double dx = (double)(out_w - rw) / 2.0;
        dx = dx - 0.1;
        double dy = (double)(out_h - rh) / 2.0;
        dy = dy - 0.1;
        x = (int32_t)rint(dx), y = (int32_t)rint(dy);
        return true;
    }
    return false;
}

// Where the job of the visible rectangle lies in the canvas.
struct Place {
    uint32_t cw, ch;  // the canvas: the batch's output size
    uint32_t vx, vy;  // the visible rectangle's first column / row in the canvas (its size is the job's out_w x out_h)
    uint32_t pre;     // bands above the first band with a visible row
    uint32_t bands;   // bands of the canvas
    int32_t row0;     // the canvas row band 0 begins at, in (-rb, 0]: band k covers rows [row0 + k rb, row0 + (k + 1) rb) of the canvas
    uint32_t shift;   // the LDS rows begin at this byte (0..15)
    uint32_t fill;    // fill[c] in byte c
};
struct PlacedJob {
    ResampleJob r;  // the visible rectangle as a job: tables of the visible range, planned over the visible rows; dst: the canvas
    Place p;
};
struct PlacedTensorJob {
    TensorJob t;  // t.r as PlacedJob::r; plane: the canvas's
    Place p;
};

// Plans the visible rectangle's job (sizes, table offsets and p.cw, p.ch, p.vx, p.vy set; `tab`: host copy of the tables) and the bands
// of the canvas.  False for what the kernel does not run.
inline bool placed_plan(ResampleJob &j, Place &p, const int32_t *tab, uint32_t lds_cap = RS_MAX_LDS, uint32_t rb_cap = 64u) {
    if (j.src_nc != 0 && (j.nc != 3 || (j.src_nc != 1 && j.src_nc != 4))) return false;
    if (j.nc == 0 || j.nc > 4 || j.in_w == 0 || j.in_h == 0 || j.out_w == 0 || j.out_h == 0) return false;
    if (p.cw == 0 || p.ch == 0 || p.cw > RS_MAX_OUT || p.ch > RS_MAX_OUT) return false;
    if (p.vx >= p.cw || j.out_w > p.cw - p.vx || p.vy >= p.ch || j.out_h > p.ch - p.vy) return false;
    p.shift = (p.vx * j.nc) & 15u;
    j.pitch = (p.shift + j.out_w * j.nc + 15u) & ~15u;
    if (lds_cap > RS_MAX_LDS) lds_cap = RS_MAX_LDS;
    j.cap_rows = lds_cap / j.pitch;
    if (j.cap_rows == 0) return false;
    if (j.cap_rows > j.in_h) j.cap_rows = j.in_h;
    j.lds_bytes = j.cap_rows * j.pitch;
    const int32_t *vb = tab + j.vb;
    uint32_t rb = rb_cap ? rb_cap : 1u;
    if (rb > j.out_h) rb = j.out_h;
    for (; rb > 1u; rb--) {  // the largest band whose source rows fit in one chunk, for every band of visible rows
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
    p.pre = (p.vy + rb - 1u) / rb;
    p.row0 = (int32_t)p.vy - (int32_t)(p.pre * rb);
    p.bands = (p.ch + p.pre * rb - p.vy + rb - 1u) / rb;
    return true;
}

#ifdef JPGPU_RS_DEVICE_BODY
struct PBand {
    // the band's canvas rows [R0, R1); `ib`: the band of the visible rectangle's job whose rows lie in it, when `vis`
    static __device__ __forceinline__ void band_of(const ResampleJob &j, const Place &p, uint32_t band, uint32_t &R0, uint32_t &R1, uint32_t &ib, bool &vis) {
        const int32_t t0 = p.row0 + (int32_t)(band * j.rb);
        R0 = t0 < 0 ? 0u : (uint32_t)t0;
        R1 = min((uint32_t)(t0 + (int32_t)j.rb), p.ch);
        ib = band - p.pre;
        vis = band >= p.pre && ib < j.bands;
    }
    static __device__ __forceinline__ bool row_visible(const ResampleJob &j, const Place &p, uint32_t row) { return row - p.vy < j.out_h; }
    static __device__ __forceinline__ bool px_visible(const ResampleJob &j, const Place &p, uint32_t px) { return px - p.vx < j.out_w; }
    static __device__ __forceinline__ uint32_t fill_of(const Place &p, uint32_t c) { return (p.fill >> (8u * c)) & 255u; }
    // the band's run of canvas bytes [a, b) (offsets from dst) and its dwords [q0, q1)
    static __device__ __forceinline__ void run_of(const ResampleJob &j, const Place &p, uint32_t band, uint32_t &a, uint32_t &b, uint32_t &q0, uint32_t &q1) {
        uint32_t R0, R1, ib;
        bool vis;
        band_of(j, p, band, R0, R1, ib, vis);
        const uint32_t rowb = p.cw * j.nc;
        a = R0 * rowb, b = R1 * rowb;
        q0 = a >> 2, q1 = (b + 3u) >> 2;
    }
    static __device__ __forceinline__ uint32_t groups_of(const ResampleJob &j, const Place &p, uint32_t band) {
        uint32_t a, b, q0, q1;
        run_of(j, p, band, a, b, q0, q1);
        return (q1 - q0 + RS_NT - 1u) / RS_NT;
    }
    // the visible columns [x0, x1) (of the job) whose horizontal pass group `group` of the band needs: a band of one row only those under
    // the group's own bytes (none: x0 == x1), a taller one every column
    static __device__ __forceinline__ void group_columns(const ResampleJob &j, const Place &p, uint32_t band, uint32_t group, uint32_t &x0, uint32_t &x1) {
        x0 = 0u, x1 = j.out_w;
        if (j.rb != 1u) return;
        uint32_t a, b, q0, q1;
        run_of(j, p, band, a, b, q0, q1);
        const uint32_t f0 = max(4u * (q0 + group * RS_NT), a), f1 = min(4u * (q0 + (group + 1u) * RS_NT), b);
        x0 = x1 = 0u;
        if (f0 >= f1) return;
        const uint32_t lo = max((f0 - a) / j.nc, p.vx), hi = min((f1 - a + j.nc - 1u) / j.nc, p.vx + j.out_w);
        if (lo < hi) x0 = lo - p.vx, x1 = hi - p.vx;
    }

    // the share of source rows [c0, c1) (in LDS) in the four sums of canvas dword q: four visible bytes of one row at an aligned LDS
    // dword a dword per tap, else the visible bytes one by one; a filled byte has no sum
    static __device__ __forceinline__ void item_sum(const ResampleJob &j, const Place &p, const JP_GLOBAL int32_t *tab, uint32_t q, uint32_t a, uint32_t b,
                                                    uint32_t c0, uint32_t c1, const uint8_t *lds, int32_t (&sum)[4]) {
        const uint32_t rowb = p.cw * j.nc, v0 = p.vx * j.nc, v1 = v0 + j.out_w * j.nc;  // a canvas row's visible bytes [v0, v1)
        const JP_GLOBAL int32_t *vb = tab + j.vb;
        const JP_GLOBAL int32_t *vk = tab + j.vk;
        const uint32_t f0 = max(4u * q, a), f1 = min(4u * q + 4u, b);  // the dword's bytes inside the band
        const uint32_t row0 = f0 / rowb, col0 = f0 - row0 * rowb;
        const uint32_t l0 = col0 - v0 + p.shift;
        if (f1 - f0 == 4u && col0 >= v0 && col0 + 4u <= v1 && row_visible(j, p, row0) && (l0 & 3u) == 0u) {
            const uint32_t r = row0 - p.vy;
            const uint32_t ymin = (uint32_t)vb[2u * r], n = (uint32_t)vb[2u * r + 1u];
            const uint32_t t0 = c0 > ymin ? c0 - ymin : 0u, t1 = min(n, c1 > ymin ? c1 - ymin : 0u);
            const JP_GLOBAL int32_t *k = vk + (size_t)r * j.vks;
            for (uint32_t t = t0; t < t1; t++) {
                const uint32_t d = *reinterpret_cast<const uint32_t *>(lds + (ymin + t - c0) * j.pitch + l0);
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
            if (!row_visible(j, p, row) || col < v0 || col >= v1) continue;
            const uint32_t r = row - p.vy, l = col - v0 + p.shift;
            const uint32_t ymin = (uint32_t)vb[2u * r], n = (uint32_t)vb[2u * r + 1u];
            const uint32_t t0 = c0 > ymin ? c0 - ymin : 0u, t1 = min(n, c1 > ymin ? c1 - ymin : 0u);
            const JP_GLOBAL int32_t *k = vk + (size_t)r * j.vks;
            int32_t s = 0;
            for (uint32_t t = t0; t < t1; t++) s += (int32_t)lds[(ymin + t - c0) * j.pitch + l] * k[t];
            sum[e] += s;
        }
    }
    // stored: a visible byte's sum rounded and clamped, a filled byte the fill of its channel; a whole dword where all four bytes are
    // the band's, else its own bytes one by one
    static __device__ __forceinline__ void item_store(const ResampleJob &j, const Place &p, uint32_t q, uint32_t a, uint32_t b, const int32_t (&sum)[4]) {
        JP_GLOBAL uint8_t *dst = (JP_GLOBAL uint8_t *)j.dst;
        const uint32_t rowb = p.cw * j.nc, ncm = 0xffffffffu / j.nc + 1u;  // (col / nc = umulhi(col, ceil(2^32 / nc)) for nc = 2..4 and col < 2^30)
        uint32_t v[4];
#pragma unroll
        for (uint32_t e = 0; e < 4; e++) {
            const uint32_t f = 4u * q + e, row = f / rowb, col = f - row * rowb, px = j.nc == 1u ? col : __umulhi(col, ncm), c = col - px * j.nc;
            const int32_t s = (sum[e] + (1 << (RS_PRECISION_BITS - 1))) >> RS_PRECISION_BITS;
            v[e] = (row_visible(j, p, row) && px_visible(j, p, px)) ? (uint32_t)(s < 0 ? 0 : (s > 255 ? 255 : s)) : fill_of(p, c);
        }
        if (4u * q >= a && 4u * q + 4u <= b) {
            reinterpret_cast<JP_GLOBAL uint32_t *>(dst)[q] = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        } else {
#pragma unroll
            for (uint32_t e = 0; e < 4; e++)
                if (4u * q + e >= a && 4u * q + e < b) dst[4u * q + e] = (uint8_t)v[e];
        }
    }

    // a band without a visible row: its bytes are the fill
    static __device__ __forceinline__ void fill_band(const ResampleJob &j, const Place &p, uint32_t band, uint32_t tid) {
        uint32_t a, b, q0, q1;
        run_of(j, p, band, a, b, q0, q1);
#pragma unroll 1
        for (uint32_t q = q0 + tid; q < q1; q += RS_NT) {
            int32_t sum[4] = {0, 0, 0, 0};
            item_store(j, p, q, a, b, sum);
        }
    }
    // vertical pass of a band whose source rows are one chunk (`ib`: the job's band): every canvas dword summed and stored
    static __device__ __forceinline__ void vstore(const ResampleJob &j, const Place &p, const JP_GLOBAL int32_t *tab, uint32_t band, uint32_t ib, uint32_t tid,
                                                  const uint8_t *lds) {
        uint32_t r0, r1, s0, s1, a, b, q0, q1;
        RBand::rows_of(j, tab, ib, r0, r1, s0, s1);
        run_of(j, p, band, a, b, q0, q1);
#pragma unroll 1
        for (uint32_t q = q0 + tid; q < q1; q += RS_NT) {
            int32_t sum[4] = {0, 0, 0, 0};
            item_sum(j, p, tab, q, a, b, s0, s1, lds, sum);
            item_store(j, p, q, a, b, sum);
        }
    }
    // the chunked path, as RBand's
    static __device__ __forceinline__ void vacc(const ResampleJob &j, const Place &p, const JP_GLOBAL int32_t *tab, uint32_t band, uint32_t ib, uint32_t chunk,
                                                uint32_t group, uint32_t tid, const uint8_t *lds, int32_t (&sum)[4]) {
        uint32_t r0, r1, s0, s1, a, b, q0, q1;
        RBand::rows_of(j, tab, ib, r0, r1, s0, s1);
        run_of(j, p, band, a, b, q0, q1);
        const uint32_t c0 = s0 + chunk * j.cap_rows, c1 = min(c0 + j.cap_rows, s1), q = q0 + group * RS_NT + tid;
        if (q < q1 && c0 < c1) item_sum(j, p, tab, q, a, b, c0, c1, lds, sum);
    }
    static __device__ __forceinline__ void vput(const ResampleJob &j, const Place &p, uint32_t band, uint32_t group, uint32_t tid, const int32_t (&sum)[4]) {
        uint32_t a, b, q0, q1;
        run_of(j, p, band, a, b, q0, q1);
        const uint32_t q = q0 + group * RS_NT + tid;
        if (q < q1) item_store(j, p, q, a, b, sum);
    }
};

// E: the element as its bits (uint32_t for f32, uint16_t for f16 / bf16)
template <class E>
struct PTBand {
    static constexpr uint32_t ES = (uint32_t)sizeof(E);
    typedef TBand<E> TB;

    static __device__ __forceinline__ bool fast(const PlacedTensorJob &t) { return ((t.p.cw | t.t.plane) & 3u) == 0u; }
    static __device__ __forceinline__ void rows_of(const PlacedTensorJob &t, uint32_t band, uint32_t &R0, uint32_t &R1) {
        uint32_t ib;
        bool vis;
        PBand::band_of(t.t.r, t.p, band, R0, R1, ib, vis);
    }
    // the canvas column an element of column x shows
    static __device__ __forceinline__ uint32_t source_col(const PlacedTensorJob &t, uint32_t x) { return t.t.flip ? t.p.cw - 1u - x : x; }
    static __device__ __forceinline__ E fill_elem(const PlacedTensorJob &t, uint32_t c, const uint8_t *lds) {
        return TB::table_of(t.t.r, lds)[c * 256u + PBand::fill_of(t.p, c)];
    }

    // ---- the canvas width and the plane pitch multiples of four: items of four pixels x NC channels ----
    // item w of the band: canvas row r, columns [x, x + 4), which show the canvas columns xs + i (xs + 3 - i with a flip); vm: bit i set
    // where pixel i of the item is visible (15: TBand's walk over whole LDS dwords)
    static __device__ __forceinline__ void fast_item(const PlacedTensorJob &t, uint32_t band, uint32_t w, uint32_t &r, uint32_t &x, uint32_t &xs, uint32_t &vm) {
        uint32_t R0, R1;
        rows_of(t, band, R0, R1);
        const uint32_t xq = t.p.cw >> 2, rr = w / xq;
        r = R0 + rr, x = 4u * (w - rr * xq);
        xs = t.t.flip ? t.p.cw - 4u - x : x;
        vm = 0u;
        if (!PBand::row_visible(t.t.r, t.p, r)) return;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) vm |= PBand::px_visible(t.t.r, t.p, t.t.flip ? xs + 3u - i : xs + i) ? 1u << i : 0u;
    }
    // the item's 4 NC sums: all four pixels visible, in the order of the LDS bytes read (mirrored with a flip); else pixel i's at [i NC, i NC + NC)
    template <uint32_t NC>
    static __device__ __forceinline__ void fast_sum(const PlacedTensorJob &t, const JP_GLOBAL int32_t *tab, uint32_t band, uint32_t w, uint32_t c0, uint32_t c1,
                                                    const uint8_t *lds, int32_t (&sum)[16]) {
        const ResampleJob &j = t.t.r;
        uint32_t r, x, xs, vm;
        fast_item(t, band, w, r, x, xs, vm);
        if (vm == 0u) return;
        uint32_t ymin, t0, t1;
        TB::taps_of(j, tab, r - t.p.vy, c0, c1, ymin, t0, t1);
        const JP_GLOBAL int32_t *k = tab + j.vk + (size_t)(r - t.p.vy) * j.vks;
        if (vm == 15u) {
            const uint8_t *p = lds + t.p.shift + (xs - t.p.vx) * NC;  // (4 NC bytes at a multiple of 4 NC: shift and pitch keep the canvas's alignment)
            for (uint32_t tt = t0; tt < t1; tt++) {
                const uint8_t *q = p + (ymin + tt - c0) * j.pitch;
                const int32_t kt = k[tt];
                uint32_t w4[4] = {0, 0, 0, 0};
                if (NC == 4u) {
                    const v4u v = *reinterpret_cast<const v4u *>(q);
                    w4[0] = v.x, w4[1] = v.y, w4[2] = v.z, w4[3] = v.w;
                } else if (NC == 2u) {
                    const v2u v = *reinterpret_cast<const v2u *>(q);
                    w4[0] = v.x, w4[1] = v.y;
                } else {
#pragma unroll
                    for (uint32_t i = 0; i < NC; i++) w4[i] = reinterpret_cast<const uint32_t *>(q)[i];
                }
#pragma unroll
                for (uint32_t b = 0; b < 4u * NC; b++) sum[b] += (int32_t)((w4[b >> 2] >> (8u * (b & 3u))) & 255u) * kt;
            }
            return;
        }
        // pixel i shows canvas column xs + i (xs + 3 - i with a flip), NC bytes at o0 + i step of an LDS row where it is visible
        const int32_t step = t.t.flip ? -(int32_t)NC : (int32_t)NC;
        const int32_t o0 = (int32_t)t.p.shift + ((int32_t)(xs - t.p.vx) + (t.t.flip ? 3 : 0)) * (int32_t)NC;
        for (uint32_t tt = t0; tt < t1; tt++) {
            const uint8_t *q = lds + (ymin + tt - c0) * j.pitch;
            const int32_t kt = k[tt];
#pragma unroll
            for (int32_t i = 0; i < 4; i++)
                if ((vm >> i) & 1u) {
#pragma unroll
                    for (int32_t c = 0; c < (int32_t)NC; c++) sum[i * (int32_t)NC + c] += (int32_t)q[o0 + i * step + c] * kt;
                }
        }
    }
    template <uint32_t NC>
    static __device__ __forceinline__ void fast_store(const PlacedTensorJob &t, uint32_t band, uint32_t w, const int32_t (&sum)[16], const uint8_t *lds) {
        const ResampleJob &j = t.t.r;
        uint32_t r, x, xs, vm;
        fast_item(t, band, w, r, x, xs, vm);
        const E *T = TB::table_of(j, lds);
        JP_GLOBAL uint8_t *dst = (JP_GLOBAL uint8_t *)j.dst;
        const bool mirrored = vm == 15u && t.t.flip;  // (the sums lie in the order of the LDS bytes)
#pragma unroll
        for (uint32_t c = 0; c < NC; c++) {
            E e[4];
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) {
                const uint32_t v = TB::round_u8(mirrored ? sum[(3u - i) * NC + c] : sum[i * NC + c]);
                e[i] = T[c * 256u + (((vm >> i) & 1u) ? v : PBand::fill_of(t.p, c))];
            }
            TB::store4(dst + ((size_t)c * t.t.plane + (size_t)r * t.p.cw + x) * ES, e);
        }
    }

    // ---- any size: items of four consecutive elements of the flat tensor ----
    static __device__ __forceinline__ void run_of(const PlacedTensorJob &t, uint32_t band, uint32_t c, uint32_t &a, uint32_t &b, uint32_t &q0, uint32_t &q1) {
        uint32_t R0, R1;
        rows_of(t, band, R0, R1);
        a = c * t.t.plane + R0 * t.p.cw, b = c * t.t.plane + R1 * t.p.cw;
        q0 = a >> 2, q1 = (b + 3u) >> 2;
    }
    static __device__ __forceinline__ bool item_of(const PlacedTensorJob &t, uint32_t band, uint32_t w, uint32_t &c, uint32_t &q, uint32_t &a, uint32_t &b) {
        for (c = 0; c < t.t.r.nc; c++) {
            uint32_t q0, q1;
            run_of(t, band, c, a, b, q0, q1);
            if (w < q1 - q0) return q = q0 + w, true;
            w -= q1 - q0;
        }
        return false;
    }
    // element f of plane c: its canvas row and the canvas column it shows; false when filled
    static __device__ __forceinline__ bool elem_of(const PlacedTensorJob &t, uint32_t c, uint32_t f, uint32_t &row, uint32_t &sc) {
        const uint32_t g = f - c * t.t.plane;
        row = g / t.p.cw;
        sc = source_col(t, g - row * t.p.cw);
        return PBand::row_visible(t.t.r, t.p, row) && PBand::px_visible(t.t.r, t.p, sc);
    }
    static __device__ __forceinline__ void item_sum(const PlacedTensorJob &t, const JP_GLOBAL int32_t *tab, uint32_t c, uint32_t q, uint32_t a, uint32_t b,
                                                    uint32_t c0, uint32_t c1, const uint8_t *lds, int32_t (&sum)[16]) {
        const ResampleJob &j = t.t.r;
        const uint32_t f0 = max(4u * q, a), f1 = min(4u * q + 4u, b);  // the item's elements inside the band's run
        const JP_GLOBAL int32_t *vk = tab + j.vk;
#pragma unroll
        for (uint32_t e = 0; e < 4; e++) {
            const uint32_t f = 4u * q + e;
            if (f < f0 || f >= f1) continue;
            uint32_t row, sc;
            if (!elem_of(t, c, f, row, sc)) continue;
            uint32_t ymin, t0, t1;
            TB::taps_of(j, tab, row - t.p.vy, c0, c1, ymin, t0, t1);
            const JP_GLOBAL int32_t *k = vk + (size_t)(row - t.p.vy) * j.vks;
            const uint32_t col = t.p.shift + (sc - t.p.vx) * j.nc + c;
            int32_t s = 0;
            for (uint32_t tt = t0; tt < t1; tt++) s += (int32_t)lds[(ymin + tt - c0) * j.pitch + col] * k[tt];
            sum[e] += s;
        }
    }
    static __device__ __forceinline__ void item_store(const PlacedTensorJob &t, uint32_t c, uint32_t q, uint32_t a, uint32_t b, const int32_t (&sum)[16],
                                                      const uint8_t *lds) {
        const E *T = TB::table_of(t.t.r, lds) + c * 256u;
        JP_GLOBAL uint8_t *dst = (JP_GLOBAL uint8_t *)t.t.r.dst;
        E e[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            const uint32_t f = 4u * q + i;
            uint32_t row, sc;
            const bool in = f >= a && f < b;
            e[i] = T[(in && elem_of(t, c, f, row, sc)) ? TB::round_u8(sum[i]) : PBand::fill_of(t.p, c)];
        }
        if (4u * q >= a && 4u * q + 4u <= b) {
            TB::store4(dst + (size_t)q * 4u * ES, e);
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 4; i++)
                if (4u * q + i >= a && 4u * q + i < b) reinterpret_cast<JP_GLOBAL E *>(dst)[4u * q + i] = e[i];
        }
    }

    // ---- the band ----
    static __device__ __forceinline__ uint32_t items_of(const PlacedTensorJob &t, uint32_t band) {
        uint32_t R0, R1;
        rows_of(t, band, R0, R1);
        if (fast(t)) return (R1 - R0) * (t.p.cw >> 2);
        uint32_t n = 0;
        for (uint32_t c = 0; c < t.t.r.nc; c++) {
            uint32_t a, b, q0, q1;
            run_of(t, band, c, a, b, q0, q1);
            n += q1 - q0;
        }
        return n;
    }
    static __device__ __forceinline__ uint32_t groups_of(const PlacedTensorJob &t, uint32_t band) { return (items_of(t, band) + RS_NT - 1u) / RS_NT; }
    // the visible columns [x0, x1) (of the job) whose horizontal pass group `group` needs: a band of one row with four-pixel items only
    // those its items show (none: x0 == x1), any other every column
    static __device__ __forceinline__ void group_columns(const PlacedTensorJob &t, uint32_t band, uint32_t group, uint32_t &x0, uint32_t &x1) {
        const ResampleJob &j = t.t.r;
        x0 = 0u, x1 = j.out_w;
        if (j.rb != 1u || !fast(t)) return;
        const uint32_t i0 = group * RS_NT, i1 = min(i0 + RS_NT, t.p.cw >> 2);
        x0 = x1 = 0u;
        if (i0 >= i1) return;
        const uint32_t s0 = t.t.flip ? t.p.cw - 4u * i1 : 4u * i0, s1 = t.t.flip ? t.p.cw - 4u * i0 : 4u * i1;
        const uint32_t lo = max(s0, t.p.vx), hi = min(s1, t.p.vx + j.out_w);
        if (lo < hi) x0 = lo - t.p.vx, x1 = hi - t.p.vx;
    }
    static __device__ __forceinline__ void sum_item(const PlacedTensorJob &t, const JP_GLOBAL int32_t *tab, uint32_t band, uint32_t w, uint32_t c0, uint32_t c1,
                                                    const uint8_t *lds, int32_t (&sum)[16]) {
        if (fast(t)) {
            switch (t.t.r.nc) {  // (uniform)
            case 1: fast_sum<1>(t, tab, band, w, c0, c1, lds, sum); break;
            case 2: fast_sum<2>(t, tab, band, w, c0, c1, lds, sum); break;
            case 3: fast_sum<3>(t, tab, band, w, c0, c1, lds, sum); break;
            default: fast_sum<4>(t, tab, band, w, c0, c1, lds, sum); break;
            }
            return;
        }
        uint32_t c, q, a, b;
        if (item_of(t, band, w, c, q, a, b)) item_sum(t, tab, c, q, a, b, c0, c1, lds, sum);
    }
    static __device__ __forceinline__ void store_item(const PlacedTensorJob &t, uint32_t band, uint32_t w, const int32_t (&sum)[16], const uint8_t *lds) {
        if (fast(t)) {
            switch (t.t.r.nc) {
            case 1: fast_store<1>(t, band, w, sum, lds); break;
            case 2: fast_store<2>(t, band, w, sum, lds); break;
            case 3: fast_store<3>(t, band, w, sum, lds); break;
            default: fast_store<4>(t, band, w, sum, lds); break;
            }
            return;
        }
        uint32_t c, q, a, b;
        if (item_of(t, band, w, c, q, a, b)) item_store(t, c, q, a, b, sum, lds);
    }

    // a band without a visible row: every element T[c][fill[c]] (the table is in LDS)
    static __device__ __forceinline__ void fill_band(const PlacedTensorJob &t, uint32_t band, uint32_t tid, const uint8_t *lds) {
        const uint32_t items = items_of(t, band);
#pragma unroll 1
        for (uint32_t w = tid; w < items; w += RS_NT) {
            int32_t sum[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            store_item(t, band, w, sum, lds);
        }
    }
    static __device__ __forceinline__ void vstore(const PlacedTensorJob &t, const JP_GLOBAL int32_t *tab, uint32_t band, uint32_t ib, uint32_t tid,
                                                  const uint8_t *lds) {
        uint32_t r0, r1, s0, s1;
        RBand::rows_of(t.t.r, tab, ib, r0, r1, s0, s1);
        const uint32_t items = items_of(t, band);
#pragma unroll 1
        for (uint32_t w = tid; w < items; w += RS_NT) {
            int32_t sum[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            sum_item(t, tab, band, w, s0, s1, lds, sum);
            store_item(t, band, w, sum, lds);
        }
    }
    static __device__ __forceinline__ void vacc(const PlacedTensorJob &t, const JP_GLOBAL int32_t *tab, uint32_t band, uint32_t ib, uint32_t chunk, uint32_t group,
                                                uint32_t tid, const uint8_t *lds, int32_t (&sum)[16]) {
        uint32_t r0, r1, s0, s1;
        RBand::rows_of(t.t.r, tab, ib, r0, r1, s0, s1);
        const uint32_t c0 = s0 + chunk * t.t.r.cap_rows, c1 = min(c0 + t.t.r.cap_rows, s1), w = group * RS_NT + tid;
        if (w < items_of(t, band) && c0 < c1) sum_item(t, tab, band, w, c0, c1, lds, sum);
    }
    static __device__ __forceinline__ void vput(const PlacedTensorJob &t, uint32_t band, uint32_t group, uint32_t tid, const int32_t (&sum)[16],
                                                const uint8_t *lds) {
        const uint32_t w = group * RS_NT + tid;
        if (w < items_of(t, band)) store_item(t, band, w, sum, lds);
    }
};
#endif  // JPGPU_RS_DEVICE_BODY

}  // namespace jpgpu

#if defined(__HIP__) && !defined(JPGPU_HOST_EMULATION)
namespace jpgpu {
// placed.hip: as launch_resample_band / launch_resample_tensor, max_bands over the jobs' canvas bands (Place::bands)
hipError_t launch_resample_placed(const PlacedJob *d_jobs, const int32_t *d_tab, uint32_t n_images, uint32_t max_bands, uint32_t lds_bytes, hipStream_t stream,
                                  bool rgb);
hipError_t launch_resample_placed_tensor(const PlacedTensorJob *d_jobs, const int32_t *d_tab, const void *d_ttab, uint32_t elem_bytes, uint32_t n_images,
                                         uint32_t max_bands, uint32_t lds_bytes, hipStream_t stream, bool rgb);
}  // namespace jpgpu
#endif
