// colour.hip — the colour kernel of jpgpu_batch_create_coloured (colour_band.hpp): one launch behind the batch's u8 resample and in
// front of its finishing (warp) launch, a workgroup per image, which walks the image's program in place.  The program is uniform in a
// workgroup; an image with an empty program leaves at once.
#include "colour_band.hpp"

namespace jpgpu {

__global__ __launch_bounds__(CL_NT) void colour_kernel(const ColourJob *__restrict__ jobs, const double *__restrict__ scale_, uint32_t n_images) {
    __shared__ ColourLds lds;
    if (blockIdx.x >= n_images) return;
    const ColourJob &j = jobs[blockIdx.x];  // (read where it lies: a private copy indexed by k would be an array in LDS per lane)
    const uint32_t n = min(j.prog.n, CL_MAX_OPS);
    for (uint32_t k = 0; k < n; k++)  // (uniform)
        for (uint32_t phase = 0; phase < CL_PHASES; phase++) {
            CBand<CL_NT>::phase(j, k, phase, (const JP_GLOBAL double *)scale_, threadIdx.x, lds);
            __syncthreads();  // (the workgroup's own stores to the image, too, are behind it)
        }
}

hipError_t launch_colour(const ColourJob *d_jobs, const double *d_scale, uint32_t n_images, hipStream_t stream) {
    if (n_images == 0) return hipSuccess;
    colour_kernel<<<dim3(n_images), dim3(CL_NT), 0, stream>>>(d_jobs, d_scale, n_images);
    return hipGetLastError();
}

}  // namespace jpgpu
