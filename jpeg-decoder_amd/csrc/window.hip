// window.hip — the window kernel of jpgpu_batch_create_windowed (window_band.hpp): one launch per scale present, every windowed
// image of the batch in it.
#include "window_band.hpp"

namespace jpgpu {

// A 1-D grid numbered for the XCDs, as scaled_fused_kernel (kernels.hip): workgroups go to the 8 XCDs round-robin, so launch slot
// s of XCD k is workgroup 8 s + k.  Column `col` = (image, tile) takes XCD col % 8 and its bands are consecutive slots there: the
// bands above and below a tile, whose rings overlap its own blocks, run side by side in one L2.  Only the windows' tiles are in
// the grid (max_tiles_x / max_bands over the images' windows); a workgroup beyond its own image's window leaves at once.
template <int SCALE>
__global__ __launch_bounds__(WB_NT) void window_band_kernel(const WindowGeom *__restrict__ geoms, const ImageJob *__restrict__ jobs,
                                                            const PlaneJob *__restrict__ planes, uint32_t max_tiles_x, uint32_t max_bands, uint32_t n_images) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, col = (slot / max_bands) * 8u + xcd, band = slot % max_bands;
    const uint32_t image = col / max_tiles_x, tile = col - image * max_tiles_x;
    if (image >= n_images) return;
    const WindowGeom &g = geoms[image];
    if (g.scale != (uint32_t)SCALE || tile >= g.tiles_x || band >= g.bands) return;  // (uniform)
    typedef WBand<SCALE> K;
    K::transform(g, planes + g.first_plane_job, tile, band, threadIdx.x, lds_raw);
    __syncthreads();
    K::pixels(g, jobs[image], tile, band, threadIdx.x, lds_raw);
}

hipError_t launch_window_band(const WindowGeom *d_geoms, const ImageJob *d_jobs, const PlaneJob *d_planes, uint32_t n_images, uint32_t max_tiles_x,
                              uint32_t max_bands, uint32_t lds_bytes, const bool (&scales)[9], hipStream_t stream) {
    if (n_images == 0 || max_tiles_x == 0 || max_bands == 0) return hipSuccess;
    const uint64_t cols = (uint64_t)n_images * max_tiles_x, wgs = ((cols + 7u) / 8u) * 8u * max_bands;
    if (wgs > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)wgs), block(WB_NT);
    if (scales[8]) window_band_kernel<8><<<grid, block, lds_bytes, stream>>>(d_geoms, d_jobs, d_planes, max_tiles_x, max_bands, n_images);
    if (scales[4]) window_band_kernel<4><<<grid, block, lds_bytes, stream>>>(d_geoms, d_jobs, d_planes, max_tiles_x, max_bands, n_images);
    if (scales[2]) window_band_kernel<2><<<grid, block, lds_bytes, stream>>>(d_geoms, d_jobs, d_planes, max_tiles_x, max_bands, n_images);
    if (scales[1]) window_band_kernel<1><<<grid, block, lds_bytes, stream>>>(d_geoms, d_jobs, d_planes, max_tiles_x, max_bands, n_images);
    return hipGetLastError();
}

}  // namespace jpgpu
