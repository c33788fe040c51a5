// resample.hip — the resample kernels of jpgpu_batch_create_resized (resample_band.hpp) and jpgpu_batch_create_tensor (tensor_band.hpp):
// one launch, every image of the batch in it.
#include "tensor_band.hpp"

namespace jpgpu {

// A 1-D grid numbered for the XCDs, as scaled_fused_kernel (kernels.hip): workgroups go to the 8 XCDs round-robin, so launch slot
// s of XCD k is workgroup 8 s + k.  Image `image` takes XCD image % 8 and its bands are consecutive slots there: neighbouring bands
// read overlapping source rows and the same tables, side by side in one L2.  A workgroup beyond its own image's bands leaves at once.
__global__ __launch_bounds__(RS_NT, 4) void resample_band_kernel(const ResampleJob *__restrict__ jobs, const int32_t *__restrict__ tab_, uint32_t max_bands,
                                                              uint32_t n_images) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, image = (slot / max_bands) * 8u + xcd, band = slot % max_bands;
    if (image >= n_images) return;
    const ResampleJob j = jobs[image];
    if (band >= j.bands) return;  // (uniform)
    const JP_GLOBAL int32_t *tab = (const JP_GLOBAL int32_t *)tab_;
    const uint32_t chunks = RBand::chunks_of(j, tab, band), tid = threadIdx.x;
    if (chunks == 1u) {  // (uniform) the band's source rows fit: one horizontal pass, every dword summed and stored
        RBand::hpass(j, tab, band, 0u, 0u, j.out_w, tid, lds_raw);
        __syncthreads();
        RBand::vstore(j, tab, band, tid, lds_raw);
        return;
    }
    const uint32_t groups = RBand::groups_of(j, band);
    for (uint32_t group = 0; group < groups; group++) {
        uint32_t x0, x1;
        RBand::group_columns(j, band, group, x0, x1);
        int32_t sum[4] = {0, 0, 0, 0};
        for (uint32_t chunk = 0; chunk < chunks; chunk++) {
            __syncthreads();  // (the vertical pass before has read its rows)
            RBand::hpass(j, tab, band, chunk, x0, x1, tid, lds_raw);
            __syncthreads();
            RBand::vacc(j, tab, band, chunk, group, tid, lds_raw, sum);
        }
        RBand::vput(j, band, group, tid, sum);
    }
}

// ---- RGB output (JPGPU_BATCH_RGB_OUTPUT) ----
// The kernel of a batch whose every image gives three channels: the same grid, bands, chunks, vertical pass and store, every job with
// nc = 3.  KIND (uniform per workgroup, the job's src_nc): 0 — a three-channel source, RBand::hpass as above; 1 / 4 — a gray / CMYK
// source whose horizontal pass converts and leaves three-channel rows in LDS (RBand::hpass_of).  The kernels above are not written
// through these bodies: their code stays what it was, instruction for instruction.
template <uint32_t KIND>
static __device__ __forceinline__ void resample_band_rgb_body(const ResampleJob *__restrict__ jobs, const int32_t *__restrict__ tab_, uint32_t max_bands,
                                                              uint32_t n_images, uint8_t *lds_raw) {
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, image = (slot / max_bands) * 8u + xcd, band = slot % max_bands;
    if (image >= n_images) return;
    const ResampleJob j = jobs[image];
    if (band >= j.bands) return;  // (uniform)
    const JP_GLOBAL int32_t *tab = (const JP_GLOBAL int32_t *)tab_;
    const uint32_t chunks = RBand::chunks_of(j, tab, band), tid = threadIdx.x;
    if (chunks == 1u) {  // (uniform)
        RBand::hpass_of<KIND>(j, tab, band, 0u, 0u, j.out_w, tid, lds_raw);
        __syncthreads();
        RBand::vstore(j, tab, band, tid, lds_raw);
        return;
    }
    const uint32_t groups = RBand::groups_of(j, band);
    for (uint32_t group = 0; group < groups; group++) {
        uint32_t x0, x1;
        RBand::group_columns(j, band, group, x0, x1);
        int32_t sum[4] = {0, 0, 0, 0};
        for (uint32_t chunk = 0; chunk < chunks; chunk++) {
            __syncthreads();  // (the vertical pass before has read its rows)
            RBand::hpass_of<KIND>(j, tab, band, chunk, x0, x1, tid, lds_raw);
            __syncthreads();
            RBand::vacc(j, tab, band, chunk, group, tid, lds_raw, sum);
        }
        RBand::vput(j, band, group, tid, sum);
    }
}
__global__ __launch_bounds__(RS_NT, 4) void resample_band_rgb_kernel(const ResampleJob *__restrict__ jobs, const int32_t *__restrict__ tab_, uint32_t max_bands,
                                                                  uint32_t n_images) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const uint32_t image = ((blockIdx.x >> 3) / max_bands) * 8u + (blockIdx.x & 7u), kind = image < n_images ? jobs[image].src_nc : 0u;  // (uniform)
    // (in this order: with the converting bodies first the register allocator spills)
    if (kind == 0u) resample_band_rgb_body<0u>(jobs, tab_, max_bands, n_images, lds_raw);
    else if (kind == 1u) resample_band_rgb_body<1u>(jobs, tab_, max_bands, n_images, lds_raw);
    else resample_band_rgb_body<4u>(jobs, tab_, max_bands, n_images, lds_raw);
}

hipError_t launch_resample_band(const ResampleJob *d_jobs, const int32_t *d_tab, uint32_t n_images, uint32_t max_bands, uint32_t lds_bytes, hipStream_t stream,
                                bool rgb) {
    if (n_images == 0 || max_bands == 0) return hipSuccess;
    if (lds_bytes > RS_MAX_LDS) return hipErrorInvalidValue;
    const uint64_t wgs = (((uint64_t)n_images + 7u) / 8u) * 8u * max_bands;
    if (wgs > 0x7fffffffull) return hipErrorInvalidValue;
    if (rgb) resample_band_rgb_kernel<<<dim3((uint32_t)wgs), dim3(RS_NT), lds_bytes, stream>>>(d_jobs, d_tab, max_bands, n_images);
    else resample_band_kernel<<<dim3((uint32_t)wgs), dim3(RS_NT), lds_bytes, stream>>>(d_jobs, d_tab, max_bands, n_images);
    return hipGetLastError();
}

// The same grid, bands, chunks and horizontal pass; the vertical pass writes the image's tensor (tensor_band.hpp).  E: the element's bits.
template <class E>
__global__ __launch_bounds__(RS_NT, 4) void resample_tensor_kernel(const TensorJob *__restrict__ jobs, const int32_t *__restrict__ tab_,
                                                                const uint32_t *__restrict__ ttab_, uint32_t max_bands, uint32_t n_images) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, image = (slot / max_bands) * 8u + xcd, band = slot % max_bands;
    if (image >= n_images) return;
    const TensorJob t = jobs[image];
    if (band >= t.r.bands) return;  // (uniform)
    const JP_GLOBAL int32_t *tab = (const JP_GLOBAL int32_t *)tab_;
    const uint32_t chunks = RBand::chunks_of(t.r, tab, band), tid = threadIdx.x;
    TBand<E>::load_table(t, (const JP_GLOBAL uint32_t *)ttab_, tid, lds_raw);
    if (chunks == 1u) {  // (uniform)
        RBand::hpass(t.r, tab, band, 0u, 0u, t.r.out_w, tid, lds_raw);
        __syncthreads();
        TBand<E>::vstore(t, tab, band, tid, lds_raw);
        return;
    }
    const uint32_t groups = TBand<E>::groups_of(t, band);
    for (uint32_t group = 0; group < groups; group++) {
        uint32_t x0, x1;
        TBand<E>::group_columns(t, band, group, x0, x1);
        int32_t sum[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t chunk = 0; chunk < chunks; chunk++) {
            __syncthreads();  // (the vertical pass before has read its rows; the table is in place)
            RBand::hpass(t.r, tab, band, chunk, x0, x1, tid, lds_raw);
            __syncthreads();
            TBand<E>::vacc(t, tab, band, chunk, group, tid, lds_raw, sum);
        }
        TBand<E>::vput(t, band, group, tid, sum, lds_raw);
    }
}

// The tensor kernel of a batch with RGB output: as resample_band_rgb_kernel, the vertical pass of resample_tensor_kernel behind it.
template <class E, uint32_t KIND>
static __device__ __forceinline__ void resample_tensor_rgb_body(const TensorJob *__restrict__ jobs, const int32_t *__restrict__ tab_,
                                                                const uint32_t *__restrict__ ttab_, uint32_t max_bands, uint32_t n_images, uint8_t *lds_raw) {
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, image = (slot / max_bands) * 8u + xcd, band = slot % max_bands;
    if (image >= n_images) return;
    const TensorJob t = jobs[image];
    if (band >= t.r.bands) return;  // (uniform)
    const JP_GLOBAL int32_t *tab = (const JP_GLOBAL int32_t *)tab_;
    const uint32_t chunks = RBand::chunks_of(t.r, tab, band), tid = threadIdx.x;
    TBand<E>::load_table(t, (const JP_GLOBAL uint32_t *)ttab_, tid, lds_raw);
    if (chunks == 1u) {  // (uniform)
        RBand::hpass_of<KIND>(t.r, tab, band, 0u, 0u, t.r.out_w, tid, lds_raw);
        __syncthreads();
        TBand<E>::vstore(t, tab, band, tid, lds_raw);
        return;
    }
    const uint32_t groups = TBand<E>::groups_of(t, band);
    for (uint32_t group = 0; group < groups; group++) {
        uint32_t x0, x1;
        TBand<E>::group_columns(t, band, group, x0, x1);
        int32_t sum[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t chunk = 0; chunk < chunks; chunk++) {
            __syncthreads();  // (the vertical pass before has read its rows; the table is in place)
            RBand::hpass_of<KIND>(t.r, tab, band, chunk, x0, x1, tid, lds_raw);
            __syncthreads();
            TBand<E>::vacc(t, tab, band, chunk, group, tid, lds_raw, sum);
        }
        TBand<E>::vput(t, band, group, tid, sum, lds_raw);
    }
}
template <class E>
__global__ __launch_bounds__(RS_NT, 4) void resample_tensor_rgb_kernel(const TensorJob *__restrict__ jobs, const int32_t *__restrict__ tab_,
                                                                    const uint32_t *__restrict__ ttab_, uint32_t max_bands, uint32_t n_images) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const uint32_t image = ((blockIdx.x >> 3) / max_bands) * 8u + (blockIdx.x & 7u), kind = image < n_images ? jobs[image].r.src_nc : 0u;  // (uniform)
    if (kind == 0u) resample_tensor_rgb_body<E, 0u>(jobs, tab_, ttab_, max_bands, n_images, lds_raw);
    else if (kind == 1u) resample_tensor_rgb_body<E, 1u>(jobs, tab_, ttab_, max_bands, n_images, lds_raw);
    else resample_tensor_rgb_body<E, 4u>(jobs, tab_, ttab_, max_bands, n_images, lds_raw);
}

hipError_t launch_resample_tensor(const TensorJob *d_jobs, const int32_t *d_tab, const void *d_ttab, uint32_t elem_bytes, uint32_t n_images, uint32_t max_bands,
                                  uint32_t lds_bytes, hipStream_t stream, bool rgb) {
    if (n_images == 0 || max_bands == 0) return hipSuccess;
    if (lds_bytes > RS_MAX_LDS || (elem_bytes != 2u && elem_bytes != 4u)) return hipErrorInvalidValue;
    const uint64_t wgs = (((uint64_t)n_images + 7u) / 8u) * 8u * max_bands;
    if (wgs > 0x7fffffffull) return hipErrorInvalidValue;
    const uint32_t lds = ((lds_bytes + 15u) & ~15u) + 4u * 256u * elem_bytes;  // the rows, then the table
    if (rgb && elem_bytes == 4u)
        resample_tensor_rgb_kernel<uint32_t><<<dim3((uint32_t)wgs), dim3(RS_NT), lds, stream>>>(d_jobs, d_tab, (const uint32_t *)d_ttab, max_bands, n_images);
    else if (rgb)
        resample_tensor_rgb_kernel<uint16_t><<<dim3((uint32_t)wgs), dim3(RS_NT), lds, stream>>>(d_jobs, d_tab, (const uint32_t *)d_ttab, max_bands, n_images);
    else if (elem_bytes == 4u)
        resample_tensor_kernel<uint32_t><<<dim3((uint32_t)wgs), dim3(RS_NT), lds, stream>>>(d_jobs, d_tab, (const uint32_t *)d_ttab, max_bands, n_images);
    else
        resample_tensor_kernel<uint16_t><<<dim3((uint32_t)wgs), dim3(RS_NT), lds, stream>>>(d_jobs, d_tab, (const uint32_t *)d_ttab, max_bands, n_images);
    return hipGetLastError();
}

}  // namespace jpgpu
