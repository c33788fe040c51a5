// placed.hip — the resample kernels of jpgpu_batch_create_placed (placed_band.hpp): the grid of resample.hip over every image's canvas
// bands.  A band without a visible row is filled here; any other goes through the walk of band_walk.hpp — the chunks and the horizontal
// passes over the image's visible rectangle, the vertical pass and the store over its canvas.  Launched for a batch with a placement
// only (jpgpu_batch_path has "+place").
#include "band_walk.hpp"

namespace jpgpu {

// KIND: as resample_band_body (0: the source has the job's channels; 1 / 4: a gray / CMYK source converted to three)
template <uint32_t KIND>
static __device__ __forceinline__ void resample_placed_body(const PlacedJob *__restrict__ jobs, const int32_t *__restrict__ tab_, uint32_t max_bands,
                                                            uint32_t n_images, uint8_t *lds_raw) {
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, image = (slot / max_bands) * 8u + xcd, band = slot % max_bands;
    if (image >= n_images) return;
    const PlacedJob *jp = jobs + image;
    const ResampleJob j = jp->r;
    uint32_t ib, shift;
    {
        const Place p = jp->p;
        if (band >= p.bands) return;  // (uniform)
        uint32_t R0, R1;
        bool vis;
        PBand::band_of(j, p, band, R0, R1, ib, vis);
        if (!vis) {  // (uniform) no visible row: the fill, and nothing read
            PBand::fill_band(j, p, band, threadIdx.x);
            return;
        }
        shift = p.shift;
    }
    DeviceLanes lanes;
    band_walk(PlacedBand<KIND>(j, jp, (const JP_GLOBAL int32_t *)tab_, band, ib, shift, lds_raw), lanes);
}
__global__ __launch_bounds__(RS_NT, 4) void resample_placed_kernel(const PlacedJob *__restrict__ jobs, const int32_t *__restrict__ tab_, uint32_t max_bands,
                                                                uint32_t n_images) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    resample_placed_body<0u>(jobs, tab_, max_bands, n_images, lds_raw);
}
__global__ __launch_bounds__(RS_NT, 4) void resample_placed_rgb_kernel(const PlacedJob *__restrict__ jobs, const int32_t *__restrict__ tab_, uint32_t max_bands,
                                                                    uint32_t n_images) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const uint32_t image = ((blockIdx.x >> 3) / max_bands) * 8u + (blockIdx.x & 7u), kind = image < n_images ? jobs[image].r.src_nc : 0u;  // (uniform)
    if (kind == 0u) resample_placed_body<0u>(jobs, tab_, max_bands, n_images, lds_raw);
    else if (kind == 1u) resample_placed_body<1u>(jobs, tab_, max_bands, n_images, lds_raw);
    else resample_placed_body<4u>(jobs, tab_, max_bands, n_images, lds_raw);
}

hipError_t launch_resample_placed(const PlacedJob *d_jobs, const int32_t *d_tab, uint32_t n_images, uint32_t max_bands, uint32_t lds_bytes, hipStream_t stream,
                                  bool rgb) {
    uint32_t wgs;
    hipError_t err;
    if (!band_grid(n_images, max_bands, lds_bytes, wgs, err)) return err;
    if (rgb) resample_placed_rgb_kernel<<<dim3(wgs), dim3(RS_NT), lds_bytes, stream>>>(d_jobs, d_tab, max_bands, n_images);
    else resample_placed_kernel<<<dim3(wgs), dim3(RS_NT), lds_bytes, stream>>>(d_jobs, d_tab, max_bands, n_images);
    return hipGetLastError();
}

template <class E, uint32_t KIND>
static __device__ __forceinline__ void resample_placed_tensor_body(const PlacedTensorJob *__restrict__ jobs, const int32_t *__restrict__ tab_,
                                                                   const uint32_t *__restrict__ ttab_, uint32_t max_bands, uint32_t n_images, uint8_t *lds_raw) {
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, image = (slot / max_bands) * 8u + xcd, band = slot % max_bands;
    if (image >= n_images) return;
    const PlacedTensorJob t = jobs[image];
    if (band >= t.p.bands) return;  // (uniform)
    uint32_t R0, R1, ib;
    bool vis;
    PBand::band_of(t.t.r, t.p, band, R0, R1, ib, vis);
    TBand<E>::load_table(t.t, (const JP_GLOBAL uint32_t *)ttab_, threadIdx.x, lds_raw);
    if (!vis) {  // (uniform) no visible row: T[c][fill[c]], and no source read
        __syncthreads();
        PTBand<E>::fill_band(t, band, threadIdx.x, lds_raw);
        return;
    }
    DeviceLanes lanes;
    band_walk(PlacedTensorBand<E, KIND>(t, (const JP_GLOBAL int32_t *)tab_, band, ib, lds_raw), lanes);
}
template <class E>
__global__ __launch_bounds__(RS_NT, 4) void resample_placed_tensor_kernel(const PlacedTensorJob *__restrict__ jobs, const int32_t *__restrict__ tab_,
                                                                       const uint32_t *__restrict__ ttab_, uint32_t max_bands, uint32_t n_images) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    resample_placed_tensor_body<E, 0u>(jobs, tab_, ttab_, max_bands, n_images, lds_raw);
}
template <class E>
__global__ __launch_bounds__(RS_NT, 4) void resample_placed_tensor_rgb_kernel(const PlacedTensorJob *__restrict__ jobs, const int32_t *__restrict__ tab_,
                                                                           const uint32_t *__restrict__ ttab_, uint32_t max_bands, uint32_t n_images) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const uint32_t image = ((blockIdx.x >> 3) / max_bands) * 8u + (blockIdx.x & 7u), kind = image < n_images ? jobs[image].t.r.src_nc : 0u;  // (uniform)
    if (kind == 0u) resample_placed_tensor_body<E, 0u>(jobs, tab_, ttab_, max_bands, n_images, lds_raw);
    else if (kind == 1u) resample_placed_tensor_body<E, 1u>(jobs, tab_, ttab_, max_bands, n_images, lds_raw);
    else resample_placed_tensor_body<E, 4u>(jobs, tab_, ttab_, max_bands, n_images, lds_raw);
}

hipError_t launch_resample_placed_tensor(const PlacedTensorJob *d_jobs, const int32_t *d_tab, const void *d_ttab, uint32_t elem_bytes, uint32_t n_images,
                                         uint32_t max_bands, uint32_t lds_bytes, hipStream_t stream, bool rgb) {
    uint32_t wgs;
    hipError_t err;
    if (!band_grid(n_images, max_bands, lds_bytes, wgs, err)) return err;
    if (elem_bytes != 2u && elem_bytes != 4u) return hipErrorInvalidValue;
    const uint32_t lds = tensor_lds(lds_bytes, elem_bytes);
    const uint32_t *tt = (const uint32_t *)d_ttab;
    if (rgb && elem_bytes == 4u) resample_placed_tensor_rgb_kernel<uint32_t><<<dim3(wgs), dim3(RS_NT), lds, stream>>>(d_jobs, d_tab, tt, max_bands, n_images);
    else if (rgb) resample_placed_tensor_rgb_kernel<uint16_t><<<dim3(wgs), dim3(RS_NT), lds, stream>>>(d_jobs, d_tab, tt, max_bands, n_images);
    else if (elem_bytes == 4u) resample_placed_tensor_kernel<uint32_t><<<dim3(wgs), dim3(RS_NT), lds, stream>>>(d_jobs, d_tab, tt, max_bands, n_images);
    else resample_placed_tensor_kernel<uint16_t><<<dim3(wgs), dim3(RS_NT), lds, stream>>>(d_jobs, d_tab, tt, max_bands, n_images);
    return hipGetLastError();
}

}  // namespace jpgpu
