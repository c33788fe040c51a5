// warp.hip — the warp kernels of jpgpu_batch_create_warped (warp_band.hpp): one launch behind the batch's u8 resample, a workgroup per
// tile of WP_NT output pixels of an image, a lane per pixel.  The job's kind (N, N-sep, B) is uniform in a workgroup.
#include "warp_band.hpp"

namespace jpgpu {

__global__ __launch_bounds__(WP_NT) void warp_u8_kernel(const WarpJob *__restrict__ jobs, const int32_t *__restrict__ tab_, uint32_t max_tiles, uint32_t n_images) {
    const uint32_t image = blockIdx.x / max_tiles, tile = blockIdx.x - image * max_tiles;
    if (image >= n_images) return;
    const WarpJob j = jobs[image];
    if (tile >= AffBand::tiles_of(j.w, j.h)) return;  // (uniform)
    AffBand::lane_u8(j, (const JP_GLOBAL int32_t *)tab_, tile, threadIdx.x);
}

template <class E>
__global__ __launch_bounds__(WP_NT) void warp_tensor_kernel(const WarpJob *__restrict__ jobs, const int32_t *__restrict__ tab_, const E *__restrict__ ttab_,
                                                           uint32_t max_tiles, uint32_t n_images) {
    const uint32_t image = blockIdx.x / max_tiles, tile = blockIdx.x - image * max_tiles;
    if (image >= n_images) return;
    const WarpJob j = jobs[image];
    if (tile >= AffBand::tiles_of(j.w, j.h)) return;  // (uniform)
    AffBand::lane_tensor<E>(j, (const JP_GLOBAL int32_t *)tab_, (const JP_GLOBAL E *)ttab_, tile, threadIdx.x);
}

hipError_t launch_warp(const WarpJob *d_jobs, const int32_t *d_tab, const void *d_ttab, uint32_t elem_bytes, uint32_t n_images, uint32_t max_tiles,
                       hipStream_t stream) {
    if (n_images == 0 || max_tiles == 0) return hipSuccess;
    if (elem_bytes != 0u && elem_bytes != 2u && elem_bytes != 4u) return hipErrorInvalidValue;
    const uint64_t wgs = (uint64_t)n_images * max_tiles;
    if (wgs > 0x7fffffffull) return hipErrorInvalidValue;
    if (elem_bytes == 0u) warp_u8_kernel<<<dim3((uint32_t)wgs), dim3(WP_NT), 0, stream>>>(d_jobs, d_tab, max_tiles, n_images);
    else if (elem_bytes == 4u) warp_tensor_kernel<uint32_t><<<dim3((uint32_t)wgs), dim3(WP_NT), 0, stream>>>(d_jobs, d_tab, (const uint32_t *)d_ttab, max_tiles, n_images);
    else warp_tensor_kernel<uint16_t><<<dim3((uint32_t)wgs), dim3(WP_NT), 0, stream>>>(d_jobs, d_tab, (const uint16_t *)d_ttab, max_tiles, n_images);
    return hipGetLastError();
}

}  // namespace jpgpu
