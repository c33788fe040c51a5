// window_band.hpp — a window of each image's output (jpgpu_batch_create_windowed) in ONE launch: coefficients in, the window's
// pixels out, packed.  The result is defined as a slice of the whole decode (Decoder::decode(), src/decoder.rs:1300-1336):
//   - a window (x, y, w, h) lies in the pixel grid of the image's output (after Decoder::scale; for one component the component's
//     size, as compute_image has it, src/decoder.rs:1310-1332);
//   - the windowed output holds exactly its rows and columns, in the image's pixel format, row pitch w * ncomp bytes:
//     interleaving colour functions give full.reshape(H, W, nc)[y:y+h, x:x+w], color_no_convert (ColorTransform None with more
//     than one component, planar within a row, src/decoder.rs:1476-1484) gives full.reshape(H, nc, W)[y:y+h, :, x:x+w].
//
// The band kernel of fused_scaled.hpp restricted to the window, with the full-size transform added:
//   1. planner (window_geom_from_job, no HIP dependency: tests/emu runs it): the band kernel's tiles of `tx` MCUs x `ry` MCU
//      rows and their rings of neighbour blocks, laid over the MCU rectangle that covers the window.  Tiles start at MCU column
//      `ox` (the window's first MCU column rounded down to `align`, so that every tile starts at a multiple of eight output
//      pixels and of four samples of every plane) and band rows at the window's first MCU row; the last tile / band ends with
//      the window's MCU rectangle.  Rings are clamped at the image's edges only: a window edge inside the image sees the real
//      neighbour samples.  Images of any size, layout, scale (8, 4, 2, 1) and window share one launch (per-image geometry).
//   2. transform: one lane per block into the components' LDS planes, as FScaled::transform.  Full size runs idct8x8<ARITH_EXACT>
//      (bit-exact for any coefficients: windowed images need no range class) with one block per lane in flight (JPGPU_WB_FULL_BPL):
//      eight 16-byte pieces per block; two in flight measured slower (211 VGPRs, 2 waves / SIMD, against 142 and 3).
//   3. pixels: units of eight output pixels at absolute multiples of eight (aligned LDS dword reads), the reference's upsamplers
//      with absolute plane coordinates (FScaled::sample8, near_far, first / last column rules); lanes mask the columns outside
//      the window and store relative to it.  4:2:0 YCbCr units that lie wholly inside the window take the packed row arithmetic
//      of the full-size walk (PixelOps::row_pixels' arithmetic, rgb420_unit).  A whole unit's bytes go out as dwords at any
//      destination alignment (store_run_any): window rows start wherever x and w put them.
#pragma once
#include <stdint.h>

#include "../../include/jpgpu.h"
#include "fused_scaled.hpp"

namespace jpgpu {

constexpr uint32_t WB_NT = FS_NT;
constexpr uint32_t WB_MAX_BLOCKS = FS_NT * FS_BLOCKS_PER_LANE;  // blocks per workgroup, rings included
constexpr uint32_t WB_MAX_LDS = 32u * 1024u;
#ifndef JPGPU_WB_FULL_BPL
#define JPGPU_WB_FULL_BPL 1  // blocks per lane in flight at full size (1: 142 VGPRs, 3 waves / SIMD; 2: 211, 2 — 12-16 % slower)
#endif

struct WindowGeom {
    uint32_t scale, ncomp, hmax, vmax;
    uint32_t mcu_w, mcu_h;          // MCUs across / down the image
    uint32_t align;                 // tiles start at multiples of `align` MCUs (1 at full size)
    uint32_t tx, ry;                // MCUs per tile (a multiple of `align`), MCU rows per band
    uint32_t ox, oy;                // MCU column / row where the first launched tile / band starts
    uint32_t ex, ey;                // end (exclusive) of the window's MCU rectangle
    uint32_t tiles_x, bands;        // launched tiles across / bands down
    uint32_t h[4], v[4];
    uint32_t halo[4];               // 1: the ring of neighbour blocks is transformed as well (fancy upsamplers)
    uint32_t block_w[4], block_h[4];
    uint32_t lds_off[4], pitch[4];  // the component's LDS plane: (ry * v + 2 halo) * scale rows of `pitch` = tx * h * scale + 2 margin bytes,
                                    // the tile's own samples from column `margin` (a ring block's samples in the margin next to them)
    uint32_t lds_bytes;
    uint32_t margin;                // 8 at full size (a ring block is eight samples wide), else 4 as in ScaledGeom
    uint32_t out_w, out_h;          // the image's output grid
    uint32_t wx, wy, ww, wh;        // the window in it
    uint32_t first_plane_job;       // index of component 0's PlaneJob in the launch's table
};

// The image's output grid: out_w x out_h, or the component's size for one component (compute_image).
inline void window_grid(const jpgpu_component *comps, uint32_t ncomp, uint32_t out_w, uint32_t out_h, uint32_t &gw, uint32_t &gh) {
    gw = ncomp == 1 ? comps[0].size_width : out_w;
    gh = ncomp == 1 ? comps[0].size_height : out_h;
}

// Plans the window (wx, wy, ww, wh) of an image build_image_job accepted (`job`); the window must lie inside the output grid.
// Returns false with `why` for a descriptor the kernel cannot run (components at different dct_scales, grids
// update_component_sizes does not make); real streams produce none (every component gets one dct_scale, src/parser.rs:120-125).
// tx_cap / ry_cap: widest tile in MCUs, most MCU rows per band.
inline bool window_geom_from_job(const jpgpu_component *comps, uint32_t ncomp, const ImageJob &job, uint32_t wx, uint32_t wy, uint32_t ww,
                                 uint32_t wh, WindowGeom &g, const char *&why, uint32_t tx_cap = 64u, uint32_t ry_cap = 8u) {
    g = WindowGeom{};
    why = "";
    if (ncomp == 0 || ncomp > 4) return why = "component count", false;
    const uint32_t scale = comps[0].dct_scale;
    if (scale != 8u && scale != 4u && scale != 2u && scale != 1u) return why = "dct_scale", false;
    uint32_t hmax = 0, vmax = 0;
    for (uint32_t c = 0; c < ncomp; c++) {
        if (comps[c].dct_scale != scale) return why = "components at different dct_scales", false;
        hmax = hmax > comps[c].horizontal_sampling_factor ? hmax : comps[c].horizontal_sampling_factor;
        vmax = vmax > comps[c].vertical_sampling_factor ? vmax : comps[c].vertical_sampling_factor;
    }
    if (hmax == 0 || vmax == 0 || hmax > 4 || vmax > 4) return why = "sampling factors", false;
    g.scale = scale, g.ncomp = ncomp, g.hmax = hmax, g.vmax = vmax;
    g.mcu_w = comps[0].block_width / comps[0].horizontal_sampling_factor;
    g.mcu_h = comps[0].block_height / comps[0].vertical_sampling_factor;
    if (g.mcu_w == 0 || g.mcu_h == 0 || g.mcu_h > 65535u) return why = "empty MCU grid", false;
    for (uint32_t c = 0; c < ncomp; c++) {
        g.h[c] = comps[c].horizontal_sampling_factor, g.v[c] = comps[c].vertical_sampling_factor;
        g.block_w[c] = comps[c].block_width, g.block_h[c] = comps[c].block_height;
        if (g.block_w[c] != g.mcu_w * g.h[c] || g.block_h[c] != g.mcu_h * g.v[c]) return why = "block grid not made by update_component_sizes", false;
        const uint32_t k = job.comp[c].kind;
        g.halo[c] = (job.color_fn != CC_GRAY && (k == UP_H2V1 || k == UP_H1V2 || k == UP_H2V2)) ? 1u : 0u;
    }
    window_grid(comps, ncomp, job.out_w, job.out_h, g.out_w, g.out_h);
    if (ww == 0 || wh == 0 || wx + ww > g.out_w || wy + wh > g.out_h) return why = "window outside the image", false;
    g.wx = wx, g.wy = wy, g.ww = ww, g.wh = wh;
    // alignment: a tile's first output pixel a multiple of 8 (pixel units), its first sample of every plane a multiple of 4
    // (aligned LDS dword reads at the same offsets as in the plane)
    g.align = 8u;
    for (uint32_t a = 1u; a < 8u; a *= 2u) {
        bool ok = (a * hmax * scale) % 8u == 0u;
        for (uint32_t c = 0; c < ncomp; c++) ok = ok && (a * g.h[c] * scale) % 4u == 0u;
        if (ok) {
            g.align = a;
            break;
        }
    }
    const uint32_t mpx = hmax * scale, mpy = vmax * scale;  // output pixels per MCU
    const uint32_t mx0 = wx / mpx, my0 = wy / mpy;
    g.ex = (wx + ww + mpx - 1u) / mpx, g.ey = (wy + wh + mpy - 1u) / mpy;
    g.ex = g.ex < g.mcu_w ? g.ex : g.mcu_w, g.ey = g.ey < g.mcu_h ? g.ey : g.mcu_h;
    g.ox = mx0 / g.align * g.align, g.oy = my0;
    const uint32_t span_x = g.ex - g.ox, span_y = g.ey - g.oy;
    auto blocks_of = [&](uint32_t te, uint32_t re) {
        uint32_t n = 0;
        for (uint32_t c = 0; c < ncomp; c++) n += (te * g.h[c] + 2u * g.halo[c]) * (re * g.v[c] + 2u * g.halo[c]);
        return n;
    };
    g.margin = scale == 8u ? 8u : 4u;
    auto lds_of = [&](uint32_t tx, uint32_t ry) {
        uint32_t off = 0;
        for (uint32_t c = 0; c < ncomp; c++) off = (off + (tx * g.h[c] * scale + 2u * g.margin) * (ry * g.v[c] + 2u * g.halo[c]) * scale + 15u) & ~15u;
        return off;
    };
    if (blocks_of(g.align, 1u) > WB_MAX_BLOCKS || lds_of(g.align, 1u) > WB_MAX_LDS) return why = "one tile of the layout exceeds the workgroup", false;
    // Tile shape: the band planner's rule (scaled_geom_from_job) over the window's MCU rectangle — fewest transform rounds of
    // WB_NT blocks for the whole rectangle, then the taller band, then fewer workgroups.
    tx_cap = tx_cap < g.align ? g.align : (tx_cap > 64u ? 64u : tx_cap);
    tx_cap -= tx_cap % g.align;
    uint32_t best_tx = g.align, best_ry = 1u;
    uint64_t best_slots = ~0ull, best_wgs = ~0ull;
    static const uint32_t kRows[] = {1u, 2u, 3u, 4u, 6u, 8u, 12u, 16u};
    for (uint32_t ry : kRows) {
        if (ry > 1u && (ry > span_y || ry > ry_cap)) break;
        for (uint32_t tx = g.align; tx <= tx_cap; tx += g.align) {
            if (blocks_of(tx, ry) > WB_MAX_BLOCKS || lds_of(tx, ry) > WB_MAX_LDS) break;
            const uint32_t full_x = span_x / tx, rest_x = span_x - full_x * tx, full_y = span_y / ry, rest_y = span_y - full_y * ry;
            uint64_t slots = 0;
            for (uint32_t ky = 0; ky < 2u; ky++)
                for (uint32_t kx = 0; kx < 2u; kx++) {
                    const uint32_t te = kx ? rest_x : tx, re = ky ? rest_y : ry;
                    const uint64_t n_of = (uint64_t)(kx ? (rest_x ? 1u : 0u) : full_x) * (ky ? (rest_y ? 1u : 0u) : full_y);
                    if (n_of && te && re) slots += n_of * ((blocks_of(te, re) + WB_NT - 1u) / WB_NT);
                }
            const uint64_t wgs = (uint64_t)(full_x + (rest_x ? 1u : 0u)) * (full_y + (rest_y ? 1u : 0u));
            if (slots < best_slots || (slots == best_slots && (ry > best_ry || wgs < best_wgs))) best_slots = slots, best_wgs = wgs, best_tx = tx, best_ry = ry;
            if (tx >= span_x) break;
        }
    }
    g.tx = best_tx, g.ry = best_ry;
    g.tiles_x = (span_x + g.tx - 1u) / g.tx;
    g.bands = (span_y + g.ry - 1u) / g.ry;
    uint32_t off = 0;
    for (uint32_t c = 0; c < ncomp; c++) {
        g.pitch[c] = g.tx * g.h[c] * scale + 2u * g.margin;
        g.lds_off[c] = off;
        off += g.pitch[c] * (g.ry * g.v[c] + 2u * g.halo[c]) * scale;
        off = (off + 15u) & ~15u;
    }
    g.lds_bytes = off;
    return true;
}

// The block rectangle [bx0, bx1) x [by0, by1) of component c that tile (tile, band) transforms: its own blocks and its ring,
// clamped to the component's plane — never to the window (WBand::transform enumerates exactly these blocks; tests/emu checks them).
__host__ __device__ inline void window_tile_blocks(const WindowGeom &g, uint32_t c, uint32_t tile, uint32_t band, int32_t &bx0, int32_t &by0, int32_t &bx1, int32_t &by1) {
    const uint32_t x0m = g.ox + tile * g.tx, my = g.oy + band * g.ry;
    const uint32_t te = g.tx < g.ex - x0m ? g.tx : g.ex - x0m, re = g.ry < g.ey - my ? g.ry : g.ey - my;
    bx0 = (int32_t)(x0m * g.h[c]) - (int32_t)g.halo[c], by0 = (int32_t)(my * g.v[c]) - (int32_t)g.halo[c];
    bx1 = (int32_t)((x0m + te) * g.h[c] + g.halo[c]), by1 = (int32_t)((my + re) * g.v[c] + g.halo[c]);
    bx0 = bx0 < 0 ? 0 : bx0, by0 = by0 < 0 ? 0 : by0;
    bx1 = bx1 > (int32_t)g.block_w[c] ? (int32_t)g.block_w[c] : bx1, by1 = by1 > (int32_t)g.block_h[c] ? (int32_t)g.block_h[c] : by1;
}

// The rows of blocks of component c that the launch's tiles can touch (the union of window_tile_blocks' rows over every tile and
// band): [r0, r1) — and the same as whole MCU rows of the frame over all components, [my0, my1): what the device entropy route has
// to leave in the coefficient arena for a windowed image (HuffSyncJob::keep_my0 / keep_my1).  No HIP dependency (tests/emu).
inline void window_kept_rows(const WindowGeom &g, uint32_t c, uint32_t &r0, uint32_t &r1) {
    const uint32_t lo = g.oy * g.v[c], hi = g.ey * g.v[c] + g.halo[c];
    r0 = lo > g.halo[c] ? lo - g.halo[c] : 0u;
    r1 = hi < g.block_h[c] ? hi : g.block_h[c];
}
inline void window_kept_mcu_rows(const WindowGeom &g, uint32_t &my0, uint32_t &my1) {
    my0 = g.mcu_h, my1 = 0u;
    for (uint32_t c = 0; c < g.ncomp; c++) {
        uint32_t r0, r1;
        window_kept_rows(g, c, r0, r1);
        const uint32_t a = r0 / g.v[c], b = (r1 + g.v[c] - 1u) / g.v[c];
        my0 = a < my0 ? a : my0, my1 = b > my1 ? b : my1;
    }
    my1 = my1 < g.mcu_h ? my1 : g.mcu_h;
}

// A run of 4 * ND bytes (d[k] holds bytes 4k .. 4k + 3, little-endian) to `o` whatever its alignment — window rows of w * 3 or
// w bytes start anywhere: aligned dword stores, and the bytes before the first / after the last 4-byte boundary one by one
// (ND - 1 dword + 4 byte stores where the unit's bytes one by one were 4 * ND stores).
template <int ND>
__device__ __forceinline__ void store_run_any(JP_GLOBAL uint8_t *o, const uint32_t (&d)[ND]) {
    const uint32_t m = (uint32_t)(uintptr_t)o & 3u;
    if (m == 0u) {
        if constexpr (ND == 6) {
            *reinterpret_cast<JP_GLOBAL v3u_a4 *>(o) = v3u{d[0], d[1], d[2]};
            *reinterpret_cast<JP_GLOBAL v3u_a4 *>(o + 12) = v3u{d[3], d[4], d[5]};
        } else {
#pragma unroll
            for (int k = 0; k < ND; k++) reinterpret_cast<JP_GLOBAL uint32_t *>(o)[k] = d[k];
        }
        return;
    }
    const uint32_t sh = 8u * (4u - m);  // 8, 16 or 24
#pragma unroll
    for (uint32_t i = 0; i < 3u; i++)
        if (i < 4u - m) o[i] = (uint8_t)(d[0] >> (8u * i));
    JP_GLOBAL uint32_t *a = reinterpret_cast<JP_GLOBAL uint32_t *>(o + (4u - m));
#pragma unroll
    for (int k = 0; k + 1 < ND; k++) a[k] = (d[k] >> sh) | (d[k + 1] << (32u - sh));
#pragma unroll
    for (uint32_t i = 0; i < 3u; i++)
        if (i < m) o[4u * ND - m + i] = (uint8_t)(d[ND - 1] >> (sh + 8u * i));
}

// PixelOps::row_pixels' arithmetic (4:2:0 YCbCr, first / last image column fixed up) for the eight pixels at column ox0, as the
// 24 output bytes (d[k]: bytes 4k .. 4k + 3) — so that window rows at any alignment keep dword stores (store_run_any)
__device__ __forceinline__ void rgb420_unit(uint32_t cw, const PixelOps<ARITH_EXACT>::TPrime (&t)[2], v2u yy, uint32_t ox0, uint32_t (&d)[6]) {
    uint32_t pk[2][4];
#pragma unroll
    for (uint32_t comp = 0; comp < 2; comp++) {
        const PixelOps<ARITH_EXACT>::TPrime &q = t[comp];
        pk[comp][0] = pk_mad3(q.tE1, q.tOm), pk[comp][1] = pk_mad3(q.tE1, q.tO1), pk[comp][2] = pk_mad3(q.tO1, q.tE1), pk[comp][3] = pk_mad3(q.tO1, q.tEp);
    }
    const uint32_t last_x = 2u * cw - 1u;
    if (ox0 == 0u || last_x - ox0 < 8u) {  // (src/upsampler.rs:213-214, 226: c = t'main >> 2 in the first / last column)
#pragma unroll
        for (uint32_t comp = 0; comp < 2; comp++) {
            if (ox0 == 0u) pk[comp][0] = (pk[comp][0] & 0xffff0000u) | ((t[comp].tE1 << 2) & 0xfff0u);
            if (last_x - ox0 < 8u) {
                const uint32_t k = last_x - ox0;
                const uint32_t tm = k == 1u ? (t[comp].tE1 & 0xffffu) : k == 3u ? (t[comp].tO1 & 0xffffu) : k == 5u ? (t[comp].tE1 >> 16) : (t[comp].tO1 >> 16);
                const uint32_t v = (tm << 2) & 0xfff0u;
                if (k == 1u) pk[comp][1] = (pk[comp][1] & 0xffff0000u) | v;
                if (k == 3u) pk[comp][3] = (pk[comp][3] & 0xffff0000u) | v;
                if (k == 5u) pk[comp][1] = (pk[comp][1] & 0x0000ffffu) | (v << 16);
                if (k == 7u) pk[comp][3] = (pk[comp][3] & 0x0000ffffu) | (v << 16);
            }
        }
    }
    RawRgb p[8];
    const w32 yb[8] = {byte_shl20<0>(yy.x), byte_shl20<1>(yy.x), byte_shl20<2>(yy.x), byte_shl20<3>(yy.x),
                       byte_shl20<0>(yy.y), byte_shl20<1>(yy.y), byte_shl20<2>(yy.y), byte_shl20<3>(yy.y)};
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) {
        const int32_t cb = (k < 4) ? ((int32_t)(pk[0][k & 3u] << 16) >> 20) : ((int32_t)pk[0][k & 3u] >> 20);
        const int32_t cr = (k < 4) ? ((int32_t)(pk[1][k & 3u] << 16) >> 20) : ((int32_t)pk[1][k & 3u] >> 20);
        p[k] = ycbcr_raw_centred(yb[k], cb, cr);
    }
    rgb4_to_12bytes(p[0], p[1], p[2], p[3], d[0], d[1], d[2]);
    rgb4_to_12bytes(p[4], p[5], p[6], p[7], d[3], d[4], d[5]);
}

template <int SCALE>
struct WBand {
    typedef FScaled<1> L;                                     // LDS view and upsamplers (View, sample8, fetch*: independent of FScaled's scale)
    static constexpr uint32_t R = (uint32_t)SCALE;            // 16-byte pieces of a block the IDCT of this size reads (rows 0 .. R-1)
    static constexpr uint32_t BPL = SCALE == 8 ? (uint32_t)JPGPU_WB_FULL_BPL : FS_BLOCKS_PER_LANE;  // blocks per lane in flight

    static __device__ __forceinline__ uint32_t txe(const WindowGeom &g, uint32_t tile) { return min(g.tx, g.ex - (g.ox + tile * g.tx)); }
    static __device__ __forceinline__ uint32_t rye(const WindowGeom &g, uint32_t band) { return min(g.ry, g.ey - (g.oy + band * g.ry)); }

    // phase 1: the tile's blocks and ring (window_tile_blocks: clamped to the planes) -> samples in the LDS planes, in rounds of
    // WB_NT * BPL blocks
    static __device__ __forceinline__ void transform(const WindowGeom &g, const PlaneJob *__restrict__ pj, uint32_t tile, uint32_t band, uint32_t tid,
                                                     uint8_t *lds) {
        const uint32_t x0m = g.ox + tile * g.tx, my = g.oy + band * g.ry;
        uint32_t total = 0;
        for (uint32_t c = 0; c < g.ncomp; c++) {
            int32_t x0, y0, x1, y1;
            window_tile_blocks(g, c, tile, band, x0, y0, x1, y1);
            total += (uint32_t)((x1 - x0) * (y1 - y0));
        }
        for (uint32_t base = 0; base < total; base += WB_NT * BPL) {
            v4u pc[BPL][R];
            uint32_t comp[BPL], at[BPL];  // component; LDS byte offset of the block's first sample (~0: no block)
#pragma unroll
            for (uint32_t i = 0; i < BPL; i++) {
                uint32_t b = base + tid + WB_NT * i, c = 0;
                at[i] = 0xffffffffu;
                comp[i] = 0;
                if (b >= total) continue;
                int32_t x0, y0, x1, y1;
                window_tile_blocks(g, 0u, tile, band, x0, y0, x1, y1);
                uint32_t nbx = (uint32_t)(x1 - x0), cnt = nbx * (uint32_t)(y1 - y0);
                while (b >= cnt) {  // (<= 3 steps)
                    b -= cnt;
                    c++;
                    window_tile_blocks(g, c, tile, band, x0, y0, x1, y1);
                    nbx = (uint32_t)(x1 - x0);
                    cnt = nbx * (uint32_t)(y1 - y0);
                }
                const uint32_t by = b / nbx, bx = b - by * nbx;
                const uint32_t gbx = (uint32_t)x0 + bx, gby = (uint32_t)y0 + by;
                comp[i] = c;
                // (LDS block row gby - (my v - halo); the tile's own blocks start at column `margin`, a left ring block ends there)
                at[i] = g.lds_off[c] + (gby + g.halo[c] - my * g.v[c]) * (uint32_t)SCALE * g.pitch[c] + g.margin + (gbx - x0m * g.h[c]) * (uint32_t)SCALE;
                const JP_GLOBAL v4u *src = (const JP_GLOBAL v4u *)(pj[c].coefs + ((size_t)gby * g.block_w[c] + (size_t)gbx) * 64u);
                // (ring blocks are read again by the neighbouring tiles at about the same time: plain loads, as in FScaled)
#pragma unroll
                for (uint32_t r = 0; r < R; r++) pc[i][r] = g.halo[c] ? src[r] : stream_load(src + r);
            }
#pragma unroll
            for (uint32_t i = 0; i < BPL; i++) {
                if (at[i] == 0xffffffffu) continue;
                const uint32_t c = comp[i];
                uint32_t cw[32];
#pragma unroll
                for (uint32_t k = 0; k < 32; k++) cw[k] = 0u;
#pragma unroll
                for (uint32_t r = 0; r < R; r++) cw[4 * r] = pc[i][r].x, cw[4 * r + 1] = pc[i][r].y, cw[4 * r + 2] = pc[i][r].z, cw[4 * r + 3] = pc[i][r].w;
                const qtab_t q = as_qtab(pj[c].qt);
                uint8_t *dst = lds + at[i];
                if constexpr (SCALE == 8) {
                    uint32_t out[16];
                    idct8x8<ARITH_EXACT>(cw, q, out);
#pragma unroll
                    for (uint32_t r = 0; r < 8; r++) {
                        *reinterpret_cast<uint32_t *>(dst + r * g.pitch[c]) = out[2 * r];
                        *reinterpret_cast<uint32_t *>(dst + r * g.pitch[c] + 4u) = out[2 * r + 1];
                    }
                } else if constexpr (SCALE == 4) {
                    uint32_t out[4];
                    idct4x4_exact(cw, q, out);
#pragma unroll
                    for (uint32_t r = 0; r < 4; r++) *reinterpret_cast<uint32_t *>(dst + r * g.pitch[c]) = out[r];
                } else if constexpr (SCALE == 2) {
                    const uint32_t o = idct2x2_exact(cw, q);
                    *reinterpret_cast<uint16_t *>(dst) = (uint16_t)(o & 0xffffu);
                    *reinterpret_cast<uint16_t *>(dst + g.pitch[c]) = (uint16_t)(o >> 16);
                } else {
                    dst[0] = (uint8_t)idct1x1_exact(cw[0], q);
                }
            }
        }
    }

    // component c's view of its LDS plane for absolute plane coordinates (FScaled::view_of with the tile's own origin)
    static __device__ __forceinline__ typename L::View view_of(const WindowGeom &g, const ImageJob &job, uint32_t c, uint32_t tile, uint32_t band) {
        const uint32_t x0m = g.ox + tile * g.tx, my = g.oy + band * g.ry;
        const uint32_t col0 = x0m * g.h[c] * (uint32_t)SCALE - g.margin, row0 = (my * g.v[c] - g.halo[c]) * (uint32_t)SCALE;  // (wrapping)
        const UpComp &u = job.comp[c];
        return typename L::View{g.lds_off[c] - (row0 * g.pitch[c] + col0), g.pitch[c], u.kind, u.hf, u.vf, u.width, u.height};
    }

    // phase 2: the pixels of the tile that lie inside the window, eight per unit, stored relative to the window
    static __device__ __forceinline__ void pixels(const WindowGeom &g, const ImageJob &job, uint32_t tile, uint32_t band, uint32_t tid, const uint8_t *lds) {
        const uint32_t te = txe(g, tile), re = rye(g, band), nc = g.ncomp, fn = job.color_fn;
        const uint32_t x0m = g.ox + tile * g.tx, my = g.oy + band * g.ry;
        const uint32_t px0 = x0m * g.hmax * (uint32_t)SCALE, py0 = my * g.vmax * (uint32_t)SCALE;
        const uint32_t cx0 = max(px0, g.wx), cx1 = min(px0 + te * g.hmax * (uint32_t)SCALE, g.wx + g.ww);
        const uint32_t cy0 = max(py0, g.wy), cy1 = min(py0 + re * g.vmax * (uint32_t)SCALE, g.wy + g.wh);
        if (cx0 >= cx1 || cy0 >= cy1) return;
        const uint32_t ux0 = cx0 & ~7u, upr = (cx1 - ux0 + 7u) / 8u, units = upr * (cy1 - cy0);
        const typename L::View v0 = view_of(g, job, 0u, tile, band), v1 = view_of(g, job, nc > 1u ? 1u : 0u, tile, band),
                               v2 = view_of(g, job, nc > 2u ? 2u : 0u, tile, band), v3 = view_of(g, job, nc > 3u ? 3u : 0u, tile, band);
        const uint32_t wx = g.wx, ww = g.ww;
        JP_GLOBAL uint8_t *out = (JP_GLOBAL uint8_t *)job.out;
        const bool packed420 = fn == CC_YCBCR && nc == 3u && v0.kind == UP_H1V1 && v1.kind == UP_H2V2 && v2.kind == UP_H2V2 && v1.width == v2.width &&
                               v1.height == v2.height;
        typedef PixelOps<ARITH_EXACT> P;
        for (uint32_t un = tid; un < units; un += WB_NT) {
            const uint32_t r = un / upr, x = ux0 + 8u * (un - r * upr), row = cy0 + r;
            const uint32_t k0 = x < wx ? wx - x : 0u, k1 = min(8u, cx1 - x);  // the unit's columns inside the window: [k0, k1)
            const size_t orow = (size_t)(row - g.wy) * ww;                      // window row, in pixels
            if (packed420 && k0 == 0u && k1 == 8u) {
                // (the packed 16-bit H2V2 + colour arithmetic of the full-size walk, first / last image column fixed up inside)
                uint32_t near, far;
                near_far(row, v1.height, near, far);
                const uint32_t jn = near * v1.pitch + (x >> 1) - 4u, jf = far * v1.pitch + (x >> 1) - 4u;
                const typename P::TPrime t[2] = {P::tprime(P::load_eo(lds + (v1.off0 + jn)), P::load_eo(lds + (v1.off0 + jf))),
                                                 P::tprime(P::load_eo(lds + (v2.off0 + jn)), P::load_eo(lds + (v2.off0 + jf)))};
                const uint32_t yo = v0.off0 + row * v0.pitch + x;
                const v2u yy = {L::dword_at(lds, yo), L::dword_at(lds, yo + 4u)};
                uint32_t d[6];
                rgb420_unit(v1.width, t, yy, x, d);
                store_run_any(out + (orow + (x - wx)) * 3u, d);
                continue;
            }
            uint32_t s[4][8];
            L::sample8(lds, v0, x, row, s[0]);
            if (nc > 1u) L::sample8(lds, v1, x, row, s[1]);
            if (nc > 2u) L::sample8(lds, v2, x, row, s[2]);
            if (nc > 3u) L::sample8(lds, v3, x, row, s[3]);
            const bool whole = k0 == 0u && k1 == 8u;
            if (fn == CC_GRAY) {
                JP_GLOBAL uint8_t *o = out + orow;  // (column x + k - wx)
                if (whole) {
                    const uint32_t d[2] = {s[0][0] | (s[0][1] << 8) | (s[0][2] << 16) | (s[0][3] << 24), s[0][4] | (s[0][5] << 8) | (s[0][6] << 16) | (s[0][7] << 24)};
                    store_run_any(o + (x - wx), d);
                } else {
#pragma unroll
                    for (uint32_t k = 0; k < 8; k++)
                        if (k >= k0 && k < k1) o[x + k - wx] = (uint8_t)s[0][k];
                }
                continue;
            }
            if (fn == CC_NONE) {  // color_no_convert: planar within the row
                if (whole) {
#pragma unroll
                    for (uint32_t c = 0; c < 4; c++)
                        if (c < nc) {
                            const uint32_t d[2] = {s[c][0] | (s[c][1] << 8) | (s[c][2] << 16) | (s[c][3] << 24), s[c][4] | (s[c][5] << 8) | (s[c][6] << 16) | (s[c][7] << 24)};
                            store_run_any(out + orow * nc + (size_t)c * ww + (x - wx), d);
                        }
                    continue;
                }
#pragma unroll
                for (uint32_t c = 0; c < 4; c++)
#pragma unroll
                    for (uint32_t k = 0; k < 8; k++)
                        if (c < nc && k >= k0 && k < k1) out[orow * nc + (size_t)c * ww + (x + k - wx)] = (uint8_t)s[c][k];
                continue;
            }
            uint32_t px[8];
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) {
                if (fn == CC_RGB) px[k] = s[0][k] | (s[1][k] << 8) | (s[2][k] << 16);
                else if (fn == CC_YCBCR) px[k] = ycbcr_to_rgb24(s[0][k], s[1][k], s[2][k]);
                else if (fn == CC_YCCK) px[k] = ycbcr_to_rgb24(s[0][k], s[1][k], s[2][k]) | ((255u - s[3][k]) << 24);
                else px[k] = (255u - s[0][k]) | ((255u - s[1][k]) << 8) | ((255u - s[2][k]) << 16) | ((255u - s[3][k]) << 24);
            }
            JP_GLOBAL uint8_t *o = out + orow * nc;  // (pixel column x + k - wx)
            if (nc == 4u) {
                if (whole) {  // (4-byte aligned whatever the window's width)
                    *reinterpret_cast<JP_GLOBAL v4u_a4 *>(o + (x - wx) * 4u) = v4u{px[0], px[1], px[2], px[3]};
                    *reinterpret_cast<JP_GLOBAL v4u_a4 *>(o + (x - wx) * 4u + 16u) = v4u{px[4], px[5], px[6], px[7]};
                } else {
#pragma unroll
                    for (uint32_t k = 0; k < 8; k++)
                        if (k >= k0 && k < k1) reinterpret_cast<JP_GLOBAL uint32_t *>(o)[x + k - wx] = px[k];
                }
            } else if (whole) {
                const uint32_t d[6] = {px[0] | (px[1] << 24), (px[1] >> 8) | (px[2] << 16), (px[2] >> 16) | (px[3] << 8),
                                       px[4] | (px[5] << 24), (px[5] >> 8) | (px[6] << 16), (px[6] >> 16) | (px[7] << 8)};
                store_run_any(o + (x - wx) * 3u, d);
            } else {
#pragma unroll
                for (uint32_t k = 0; k < 8; k++)
                    if (k >= k0 && k < k1) {
                        JP_GLOBAL uint8_t *d = o + (x + k - wx) * 3u;
                        d[0] = (uint8_t)px[k];
                        d[1] = (uint8_t)(px[k] >> 8);
                        d[2] = (uint8_t)(px[k] >> 16);
                    }
            }
        }
    }
};

}  // namespace jpgpu

#ifndef JPGPU_HOST_EMULATION
#include <hip/hip_runtime.h>
namespace jpgpu {
// window.hip: n_images geometries / jobs (job.out = the window's output), PlaneJobs indexed by WindowGeom::first_plane_job;
// max_tiles_x / max_bands over the images' windows; scales[s]: some image of the launch decodes at dct_scale s (one launch per scale)
hipError_t launch_window_band(const WindowGeom *d_geoms, const ImageJob *d_jobs, const PlaneJob *d_planes, uint32_t n_images, uint32_t max_tiles_x,
                              uint32_t max_bands, uint32_t lds_bytes, const bool (&scales)[9], hipStream_t stream);
}  // namespace jpgpu
#endif
