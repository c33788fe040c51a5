// colour.hip — the colour kernel of jpgpu_batch_create_coloured and jpgpu_colour_apply (colour_band.hpp, colour_pixel_band.hpp): one
// launch behind the batch's u8 resample and in front of its finishing (warp) launch, a workgroup per image, which walks the image's
// program in place.  The program is uniform in a workgroup; an image with an empty program leaves at once.
#include "colour_pixel_band.hpp"

namespace jpgpu {

__global__ __launch_bounds__(CL_NT) void colour_kernel(const ColourJob *__restrict__ jobs, const double *__restrict__ scale_, uint32_t n_images, uint32_t strip_rows) {
    __shared__ ColourLds lds;
    __shared__ ColourStripLds strip;
    if (blockIdx.x >= n_images) return;
    const ColourJob &j = jobs[blockIdx.x];  // (read where it lies: a private copy indexed by k would be an array in LDS per lane)
    const uint32_t n = min(j.prog.n, CL_MAX_OPS), K = cl_strip_rows(j.w, strip_rows);
    for (uint32_t k = 0; k < n; k++) {  // (uniform, as the step counts: they depend on the job and K alone)
        const uint32_t steps = cl_op_steps(j.prog.ops[k].op, j.w, j.h, K);
        for (uint32_t step = 0; step < steps; step++) {
            CPixelBand<CL_NT>::step(j, k, step, K, (const JP_GLOBAL double *)scale_, threadIdx.x, lds, strip);
            __syncthreads();  // (the workgroup's own stores to the image, too, are behind it)
        }
    }
}

hipError_t launch_colour(const ColourJob *d_jobs, const double *d_scale, uint32_t n_images, uint32_t strip_rows, hipStream_t stream) {
    if (n_images == 0) return hipSuccess;
    colour_kernel<<<dim3(n_images), dim3(CL_NT), 0, stream>>>(d_jobs, d_scale, n_images, strip_rows);
    return hipGetLastError();
}

}  // namespace jpgpu
