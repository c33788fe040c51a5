// orient_band.hpp — the EXIF orientation in front of the fixed output size (jpgpu_batch_create_oriented).  With S what
// an image gives the resample — its source window, h x w x nc bytes, interleaved and packed — the oriented image O is Pillow's
// Image.transpose(method) under ImageOps.exif_transpose's mapping (H, W: S's size):
//     o  Pillow            O's size   O[y][x]
//     1  none              W x H      S[y][x]
//     2  FLIP_LEFT_RIGHT   W x H      S[y][W-1-x]
//     3  ROTATE_180        W x H      S[H-1-y][W-1-x]
//     4  FLIP_TOP_BOTTOM   W x H      S[H-1-y][x]
//     5  TRANSPOSE         H x W      S[x][y]
//     6  ROTATE_270        H x W      S[H-1-x][y]
//     7  TRANSVERSE        H x W      S[H-1-x][W-1-y]
//     8  ROTATE_90         H x W      S[x][W-1-y]
// Three bits state the table: the axes swap (o >= 5), S's columns run backwards (2, 3, 7, 8), S's rows run backwards (3, 4, 6, 7).
// A window of O is the same orientation of a window of S (orient_source_window): the pixel routes decode that source window as ever,
// and one launch behind them rewrites it, oriented and packed, into an arena of its own, which the image's resample job then reads.
//
// The kernel: a workgroup owns a tile of OR_T x OR_T source pixels.  It reads the tile's rows as aligned dwords into LDS (rows keep
// their byte phase; the pitch of 65 dwords is odd, so the lanes of a transposed read — consecutive source rows — fall on different
// banks), and after one barrier every lane builds aligned dwords of the tile's destination rows from LDS bytes.  A destination dword
// whose four bytes lie inside the tile's span of the row is stored whole; one it shares — with the neighbour tile or the next row —
// byte by byte, each owner its own bytes: no two stores ever touch the same byte, no dword is stored by two workgroups.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__) || defined(JPGPU_HOST_EMULATION)
#define JPGPU_OR_DEVICE_BODY 1
#include "pixel_math.hpp"
#endif

namespace jpgpu {

constexpr uint32_t OR_T = 64;         // the tile's side in source pixels
constexpr uint32_t OR_NT = 256;       // lanes of a workgroup
constexpr uint32_t OR_PITCH_DW = 65;  // dwords of a tile row in LDS: a byte phase of 0..3 and OR_T * 4 bytes; odd
constexpr uint32_t OR_LDS_DW = OR_T * OR_PITCH_DW;

#if defined(__HIP__)
#define JP_OR_BOTH __host__ __device__
#else
#define JP_OR_BOTH
#endif
inline bool orient_valid(uint32_t o) { return o >= 1u && o <= 8u; }
JP_OR_BOTH inline bool orient_swaps(uint32_t o) { return o >= 5u; }
JP_OR_BOTH inline bool orient_flips_x(uint32_t o) { return o == 2u || o == 3u || o == 7u || o == 8u; }  // (S's columns run backwards)
JP_OR_BOTH inline bool orient_flips_y(uint32_t o) { return o == 3u || o == 4u || o == 6u || o == 7u; }  // (S's rows run backwards)

// O's size for a source of w x h
inline void oriented_size(uint32_t o, uint32_t w, uint32_t h, uint32_t &ow, uint32_t &oh) {
    ow = orient_swaps(o) ? h : w, oh = orient_swaps(o) ? w : h;
}
// The window (x, y, ww, wh) of O, for a source of w x h, as the window of S whose orientation it is.  A window with ww == 0 or
// wh == 0 is the whole image and stays one; false: the window does not lie inside O.
inline bool orient_source_window(uint32_t o, uint32_t w, uint32_t h, uint32_t x, uint32_t y, uint32_t ww, uint32_t wh, uint32_t &sx, uint32_t &sy, uint32_t &sw,
                                 uint32_t &sh) {
    uint32_t ow, oh;
    oriented_size(o, w, h, ow, oh);
    if (ww == 0u || wh == 0u) return sx = sy = sw = sh = 0u, true;
    if ((uint64_t)x + ww > ow || (uint64_t)y + wh > oh) return false;
    // along S's columns and rows: the window's extent there, counted from O's origin
    const uint32_t cx = orient_swaps(o) ? y : x, cw = orient_swaps(o) ? wh : ww, ry = orient_swaps(o) ? x : y, rh = orient_swaps(o) ? ww : wh;
    sw = cw, sh = rh;
    sx = orient_flips_x(o) ? w - cx - cw : cx;
    sy = orient_flips_y(o) ? h - ry - rh : ry;
    return true;
}

// One oriented image of the launch.  src: S, h x w x nc bytes; dst: O, packed.  Both 4-byte aligned (the arenas' offsets are 256-byte
// aligned); rows start at any byte phase.
struct OrientJob {
    const uint8_t *src;
    uint8_t *dst;
    uint32_t w, h, nc, o;
    uint32_t tiles_x, tiles;
};
inline void orient_job_tiles(OrientJob &j) {
    j.tiles_x = (j.w + OR_T - 1u) / OR_T;
    j.tiles = j.tiles_x * ((j.h + OR_T - 1u) / OR_T);
}
inline size_t orient_bytes(uint32_t w, uint32_t h, uint32_t nc) { return (size_t)w * h * nc; }

#ifdef JPGPU_OR_DEVICE_BODY
struct OrientStores {
    __device__ __forceinline__ void dword(uintptr_t p, uint32_t v) const { *reinterpret_cast<JP_GLOBAL uint32_t *>(p) = v; }
    __device__ __forceinline__ void byte(uintptr_t p, uint8_t v) const { *reinterpret_cast<JP_GLOBAL uint8_t *>(p) = v; }
};
template <uint32_t NC>
struct OBand {
    // tile `tile` of the job: source rows [r0, r0 + th), columns [c0, c0 + tw)
    static __device__ __forceinline__ void tile_of(const OrientJob &j, uint32_t tile, uint32_t &r0, uint32_t &c0, uint32_t &th, uint32_t &tw) {
        const uint32_t ty = tile / j.tiles_x, tx = tile - ty * j.tiles_x;
        r0 = ty * OR_T, c0 = tx * OR_T;
        th = min(OR_T, j.h - r0), tw = min(OR_T, j.w - c0);
    }
    // address of the tile's row r in S
    static __device__ __forceinline__ uintptr_t row_address(const OrientJob &j, uint32_t r0, uint32_t c0, uint32_t r) {
        return (uintptr_t)j.src + (size_t)(r0 + r) * ((size_t)j.w * NC) + (size_t)c0 * NC;
    }

    // The tile's rows into LDS, aligned dword by aligned dword: row r at dword r * OR_PITCH_DW, its first pixel at byte (address & 3).
    // (The dwords at a row's ends hold up to three bytes of the neighbours: inside the image's 256-byte aligned slot of the arena.)
    static __device__ __forceinline__ void load(const OrientJob &j, uint32_t tile, uint32_t tid, uint32_t *lds) {
        uint32_t r0, c0, th, tw;
        tile_of(j, tile, r0, c0, th, tw);
        for (uint32_t it = tid; it < th * OR_PITCH_DW; it += OR_NT) {
            const uint32_t r = it / OR_PITCH_DW, k = it - r * OR_PITCH_DW;
            const uintptr_t a = row_address(j, r0, c0, r), p = (a & ~(uintptr_t)3) + 4u * k;
            if (p < a + tw * NC) lds[it] = *reinterpret_cast<const JP_GLOBAL uint32_t *>(p);
        }
    }

    // The tile's destination rows out of LDS.  A destination row of the tile is `dtw` pixels at column dx0: the aligned dwords that
    // cover its bytes, a lane per dword.  `st` stores (OrientStores on the device; the CPU emulation counts every byte's stores).
    template <class ST>
    static __device__ __forceinline__ void store(const OrientJob &j, uint32_t tile, uint32_t tid, const uint32_t *lds, const ST &st) {
        uint32_t r0, c0, th, tw;
        tile_of(j, tile, r0, c0, th, tw);
        const bool swap = orient_swaps(j.o), fx = orient_flips_x(j.o), fy = orient_flips_y(j.o);  // (uniform)
        // where the tile's source rows and columns go, counted along the destination
        const uint32_t a0 = fy ? j.h - r0 - th : r0, b0 = fx ? j.w - c0 - tw : c0;
        const uint32_t dx0 = swap ? a0 : b0, dtw = swap ? th : tw, dy0 = swap ? b0 : a0, dth = swap ? tw : th;
        const size_t dpitch = (size_t)(swap ? j.h : j.w) * NC;
        const uint32_t phase0 = (uint32_t)(row_address(j, r0, c0, 0u) & 3u), step = (j.w * NC) & 3u;  // (row r's byte phase: phase0 + r * step, mod 4)
        const uint8_t *ldsb = reinterpret_cast<const uint8_t *>(lds);
        for (uint32_t it = tid; it < dth * OR_PITCH_DW; it += OR_NT) {
            const uint32_t ly = it / OR_PITCH_DW, k = it - ly * OR_PITCH_DW;
            const uintptr_t d = (uintptr_t)j.dst + (size_t)(dy0 + ly) * dpitch + (size_t)dx0 * NC, end = d + dtw * NC;
            const uintptr_t p = (d & ~(uintptr_t)3) + 4u * k;
            if (p >= end) continue;
            uint32_t v = 0u, own = 0u;
#pragma unroll
            for (uint32_t b = 0; b < 4u; b++) {
                if (p + b < d || p + b >= end) continue;
                const uint32_t q = (uint32_t)(p + b - d), lx = q / NC, ch = q - lx * NC;
                const uint32_t r = swap ? (fy ? th - 1u - lx : lx) : (fy ? th - 1u - ly : ly);
                const uint32_t c = swap ? (fx ? tw - 1u - ly : ly) : (fx ? tw - 1u - lx : lx);
                v |= (uint32_t)ldsb[r * (OR_PITCH_DW * 4u) + ((phase0 + r * step) & 3u) + c * NC + ch] << (8u * b);
                own |= 1u << b;
            }
            if (own == 15u) {
                st.dword(p, v);
                continue;
            }
#pragma unroll
            for (uint32_t b = 0; b < 4u; b++)
                if (own & (1u << b)) st.byte(p + b, (uint8_t)(v >> (8u * b)));
        }
    }
};
#endif  // JPGPU_OR_DEVICE_BODY

}  // namespace jpgpu

#if defined(__HIP__) && !defined(JPGPU_HOST_EMULATION)
namespace jpgpu {
// orient.hip: n_jobs jobs of at most max_tiles tiles each, on `stream`
hipError_t launch_orient(const OrientJob *d_jobs, uint32_t n_jobs, uint32_t max_tiles, hipStream_t stream);
}  // namespace jpgpu
#endif
