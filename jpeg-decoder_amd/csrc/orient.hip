// orient.hip — the orientation kernel of jpgpu_batch_create_oriented (orient_band.hpp): one launch behind the batch's pixel launches and
// in front of its resample launch, a job per image whose orientation is not 1, a workgroup per tile of OR_T x OR_T source pixels.
#include "band_walk.hpp"
#include "orient_band.hpp"

namespace jpgpu {

// The grid is numbered for the XCDs as resample_band_kernel's (resample.hip): job `job` takes XCD job % 8 and its tiles are consecutive
// slots there — neighbouring tiles share the lines at their edges, in one L2.  A workgroup beyond its job's tiles leaves at once.
template <uint32_t NC>
static __device__ __forceinline__ void orient_body(const OrientJob &j, uint32_t tile, uint32_t *lds) {
    OBand<NC>::load(j, tile, threadIdx.x, lds);
    __syncthreads();
    OBand<NC>::store(j, tile, threadIdx.x, lds, OrientStores());
}
__global__ __launch_bounds__(OR_NT) void orient_kernel(const OrientJob *__restrict__ jobs, uint32_t max_tiles, uint32_t n_jobs) {
    __shared__ uint32_t lds[OR_LDS_DW];
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, job = (slot / max_tiles) * 8u + xcd, tile = slot % max_tiles;
    if (job >= n_jobs) return;
    const OrientJob j = jobs[job];
    if (tile >= j.tiles) return;  // (uniform)
    if (j.nc == 3u) orient_body<3u>(j, tile, lds);  // (uniform)
    else if (j.nc == 1u) orient_body<1u>(j, tile, lds);
    else orient_body<4u>(j, tile, lds);
}

hipError_t launch_orient(const OrientJob *d_jobs, uint32_t n_jobs, uint32_t max_tiles, hipStream_t stream) {
    uint32_t wgs;
    hipError_t err;
    if (!band_grid(n_jobs, max_tiles, 0u, wgs, err)) return err;
    orient_kernel<<<dim3(wgs), dim3(OR_NT), 0, stream>>>(d_jobs, max_tiles, n_jobs);
    return hipGetLastError();
}

}  // namespace jpgpu
