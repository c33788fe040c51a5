// placed.hip — the resample kernels of jpgpu_batch_create_placed (placed_band.hpp): the grid, the chunks and the horizontal passes of
// resample.hip over every image's visible rectangle, the bands, the vertical pass and the store over its canvas.  Launched for a batch
// with a placement only (jpgpu_batch_path has "+place"): resample.hip's kernels stay what they are.
#include "placed_band.hpp"

namespace jpgpu {

// The job's placement, loaded where it is used: the compiler does not carry it from an earlier load.
static __device__ __forceinline__ Place place_again(const PlacedJob *jp) {
    asm volatile("" : "+s"(jp));
    return jp->p;
}

// KIND: as resample_band_rgb_body (0: the source has the job's channels; 1 / 4: a gray / CMYK source converted to three)
template <uint32_t KIND>
static __device__ __forceinline__ void resample_placed_body(const PlacedJob *__restrict__ jobs, const int32_t *__restrict__ tab_, uint32_t max_bands,
                                                            uint32_t n_images, uint8_t *lds_raw) {
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, image = (slot / max_bands) * 8u + xcd, band = slot % max_bands;
    if (image >= n_images) return;
    const PlacedJob *jp = jobs + image;
    const ResampleJob j = jp->r;
    const uint32_t tid = threadIdx.x;
    uint32_t ib, shift;
    {
        const Place p = jp->p;
        if (band >= p.bands) return;  // (uniform)
        uint32_t R0, R1;
        bool vis;
        PBand::band_of(j, p, band, R0, R1, ib, vis);
        if (!vis) {  // (uniform) no visible row: the fill, and nothing read
            PBand::fill_band(j, p, band, tid);
            return;
        }
        shift = p.shift;
    }
    // (the placement is read again behind every horizontal pass: kept in registers across it, the kernel spills)
    const JP_GLOBAL int32_t *tab = (const JP_GLOBAL int32_t *)tab_;
    uint8_t *rows = lds_raw + shift;
    const uint32_t chunks = RBand::chunks_of(j, tab, ib);
    if (chunks == 1u) {  // (uniform)
        RBand::hpass_of<KIND>(j, tab, ib, 0u, 0u, j.out_w, tid, rows);
        __syncthreads();
        PBand::vstore(j, place_again(jp), tab, band, ib, tid, lds_raw);
        return;
    }
    const uint32_t groups = PBand::groups_of(j, place_again(jp), band);
    for (uint32_t group = 0; group < groups; group++) {
        uint32_t x0, x1;
        PBand::group_columns(j, place_again(jp), band, group, x0, x1);
        int32_t sum[4] = {0, 0, 0, 0};
        for (uint32_t chunk = 0; chunk < chunks; chunk++) {
            __syncthreads();  // (the vertical pass before has read its rows)
            RBand::hpass_of<KIND>(j, tab, ib, chunk, x0, x1, tid, rows);
            __syncthreads();
            PBand::vacc(j, place_again(jp), tab, band, ib, chunk, group, tid, lds_raw, sum);
        }
        PBand::vput(j, place_again(jp), band, group, tid, sum);
    }
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
    if (n_images == 0 || max_bands == 0) return hipSuccess;
    if (lds_bytes > RS_MAX_LDS) return hipErrorInvalidValue;
    const uint64_t wgs = (((uint64_t)n_images + 7u) / 8u) * 8u * max_bands;
    if (wgs > 0x7fffffffull) return hipErrorInvalidValue;
    if (rgb) resample_placed_rgb_kernel<<<dim3((uint32_t)wgs), dim3(RS_NT), lds_bytes, stream>>>(d_jobs, d_tab, max_bands, n_images);
    else resample_placed_kernel<<<dim3((uint32_t)wgs), dim3(RS_NT), lds_bytes, stream>>>(d_jobs, d_tab, max_bands, n_images);
    return hipGetLastError();
}

template <class E, uint32_t KIND>
static __device__ __forceinline__ void resample_placed_tensor_body(const PlacedTensorJob *__restrict__ jobs, const int32_t *__restrict__ tab_,
                                                                   const uint32_t *__restrict__ ttab_, uint32_t max_bands, uint32_t n_images, uint8_t *lds_raw) {
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, image = (slot / max_bands) * 8u + xcd, band = slot % max_bands;
    if (image >= n_images) return;
    const PlacedTensorJob t = jobs[image];
    if (band >= t.p.bands) return;  // (uniform)
    const ResampleJob &j = t.t.r;
    const uint32_t tid = threadIdx.x;
    uint32_t R0, R1, ib;
    bool vis;
    PBand::band_of(j, t.p, band, R0, R1, ib, vis);
    TBand<E>::load_table(t.t, (const JP_GLOBAL uint32_t *)ttab_, tid, lds_raw);
    if (!vis) {  // (uniform) no visible row: T[c][fill[c]], and no source read
        __syncthreads();
        PTBand<E>::fill_band(t, band, tid, lds_raw);
        return;
    }
    const JP_GLOBAL int32_t *tab = (const JP_GLOBAL int32_t *)tab_;
    uint8_t *rows = lds_raw + t.p.shift;
    const uint32_t chunks = RBand::chunks_of(j, tab, ib);
    if (chunks == 1u) {  // (uniform)
        RBand::hpass_of<KIND>(j, tab, ib, 0u, 0u, j.out_w, tid, rows);
        __syncthreads();
        PTBand<E>::vstore(t, tab, band, ib, tid, lds_raw);
        return;
    }
    const uint32_t groups = PTBand<E>::groups_of(t, band);
    for (uint32_t group = 0; group < groups; group++) {
        uint32_t x0, x1;
        PTBand<E>::group_columns(t, band, group, x0, x1);
        int32_t sum[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t chunk = 0; chunk < chunks; chunk++) {
            __syncthreads();  // (the vertical pass before has read its rows; the table is in place)
            RBand::hpass_of<KIND>(j, tab, ib, chunk, x0, x1, tid, rows);
            __syncthreads();
            PTBand<E>::vacc(t, tab, band, ib, chunk, group, tid, lds_raw, sum);
        }
        PTBand<E>::vput(t, band, group, tid, sum, lds_raw);
    }
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
    if (n_images == 0 || max_bands == 0) return hipSuccess;
    if (lds_bytes > RS_MAX_LDS || (elem_bytes != 2u && elem_bytes != 4u)) return hipErrorInvalidValue;
    const uint64_t wgs = (((uint64_t)n_images + 7u) / 8u) * 8u * max_bands;
    if (wgs > 0x7fffffffull) return hipErrorInvalidValue;
    const uint32_t lds = ((lds_bytes + 15u) & ~15u) + 4u * 256u * elem_bytes;  // the rows, then the table
    const uint32_t *tt = (const uint32_t *)d_ttab;
    if (rgb && elem_bytes == 4u) resample_placed_tensor_rgb_kernel<uint32_t><<<dim3((uint32_t)wgs), dim3(RS_NT), lds, stream>>>(d_jobs, d_tab, tt, max_bands, n_images);
    else if (rgb) resample_placed_tensor_rgb_kernel<uint16_t><<<dim3((uint32_t)wgs), dim3(RS_NT), lds, stream>>>(d_jobs, d_tab, tt, max_bands, n_images);
    else if (elem_bytes == 4u) resample_placed_tensor_kernel<uint32_t><<<dim3((uint32_t)wgs), dim3(RS_NT), lds, stream>>>(d_jobs, d_tab, tt, max_bands, n_images);
    else resample_placed_tensor_kernel<uint16_t><<<dim3((uint32_t)wgs), dim3(RS_NT), lds, stream>>>(d_jobs, d_tab, tt, max_bands, n_images);
    return hipGetLastError();
}

}  // namespace jpgpu
