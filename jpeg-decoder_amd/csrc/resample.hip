// resample.hip — the resample kernels of jpgpu_batch_create_resized (resample_band.hpp) and jpgpu_batch_create_tensor (tensor_band.hpp):
// one launch, every image of the batch in it.  A kernel is a prologue — the grid, the job, the table — in front of the one walk of
// band_walk.hpp; resample_tensor_kernel alone has the walk written out.
#include "band_walk.hpp"

namespace jpgpu {

// A 1-D grid numbered for the XCDs, as scaled_fused_kernel (kernels.hip): workgroups go to the 8 XCDs round-robin, so launch slot
// s of XCD k is workgroup 8 s + k.  Image `image` takes XCD image % 8 and its bands are consecutive slots there: neighbouring bands
// read overlapping source rows and the same tables, side by side in one L2.  A workgroup beyond its own image's bands leaves at once.
// The band itself is band_walk's (band_walk.hpp).  KIND (uniform per workgroup, the job's src_nc): 0 — the source has the job's
// channels, RBand::hpass; 1 / 4 (RGB output, JPGPU_BATCH_RGB_OUTPUT, DESIGN.md §4.12: every job has nc = 3) — a gray / CMYK source
// whose horizontal pass converts and leaves three-channel rows in LDS (RBand::hpass_of).
template <uint32_t KIND>
static __device__ __forceinline__ void resample_band_body(const ResampleJob *__restrict__ jobs, const int32_t *__restrict__ tab_, uint32_t max_bands,
                                                          uint32_t n_images, uint8_t *lds_raw) {
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, image = (slot / max_bands) * 8u + xcd, band = slot % max_bands;
    if (image >= n_images) return;
    const ResampleJob j = jobs[image];
    if (band >= j.bands) return;  // (uniform)
    DeviceLanes lanes;
    band_walk(U8Band<KIND>(j, (const JP_GLOBAL int32_t *)tab_, band, lds_raw), lanes);
}
__global__ __launch_bounds__(RS_NT, 4) void resample_band_kernel(const ResampleJob *__restrict__ jobs, const int32_t *__restrict__ tab_, uint32_t max_bands,
                                                              uint32_t n_images) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    resample_band_body<0u>(jobs, tab_, max_bands, n_images, lds_raw);
}
// The kernel of a batch with RGB output.
__global__ __launch_bounds__(RS_NT, 4) void resample_band_rgb_kernel(const ResampleJob *__restrict__ jobs, const int32_t *__restrict__ tab_, uint32_t max_bands,
                                                                  uint32_t n_images) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const uint32_t image = ((blockIdx.x >> 3) / max_bands) * 8u + (blockIdx.x & 7u), kind = image < n_images ? jobs[image].src_nc : 0u;  // (uniform)
    // (in this order: with the converting bodies first the register allocator spills)
    if (kind == 0u) resample_band_body<0u>(jobs, tab_, max_bands, n_images, lds_raw);
    else if (kind == 1u) resample_band_body<1u>(jobs, tab_, max_bands, n_images, lds_raw);
    else resample_band_body<4u>(jobs, tab_, max_bands, n_images, lds_raw);
}

hipError_t launch_resample_band(const ResampleJob *d_jobs, const int32_t *d_tab, uint32_t n_images, uint32_t max_bands, uint32_t lds_bytes, hipStream_t stream,
                                bool rgb) {
    uint32_t wgs;
    hipError_t err;
    if (!band_grid(n_images, max_bands, lds_bytes, wgs, err)) return err;
    if (rgb) resample_band_rgb_kernel<<<dim3(wgs), dim3(RS_NT), lds_bytes, stream>>>(d_jobs, d_tab, max_bands, n_images);
    else resample_band_kernel<<<dim3(wgs), dim3(RS_NT), lds_bytes, stream>>>(d_jobs, d_tab, max_bands, n_images);
    return hipGetLastError();
}

// The same grid, bands, chunks and horizontal pass; the vertical pass writes the image's tensor (tensor_band.hpp).  E: the element's bits.
template <class E, uint32_t KIND>
static __device__ __forceinline__ void resample_tensor_body(const TensorJob *__restrict__ jobs, const int32_t *__restrict__ tab_,
                                                            const uint32_t *__restrict__ ttab_, uint32_t max_bands, uint32_t n_images, uint8_t *lds_raw) {
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, image = (slot / max_bands) * 8u + xcd, band = slot % max_bands;
    if (image >= n_images) return;
    const TensorJob t = jobs[image];
    if (band >= t.r.bands) return;  // (uniform)
    TBand<E>::load_table(t, (const JP_GLOBAL uint32_t *)ttab_, threadIdx.x, lds_raw);
    DeviceLanes lanes;
    band_walk(TensorBand<E, KIND>(t, (const JP_GLOBAL int32_t *)tab_, band, lds_raw), lanes);
}
// The tensor kernel of a batch without RGB output keeps a body of its own: band_walk with TensorBand<E, 0> written out.  Through the
// shared body its f16 instance was 0.05 - 0.2 % slower than before in both series of profiles/band_walk/README.md, the project's bar.
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
// The tensor kernel of a batch with RGB output: the horizontal passes of resample_band_rgb_kernel.
template <class E>
__global__ __launch_bounds__(RS_NT, 4) void resample_tensor_rgb_kernel(const TensorJob *__restrict__ jobs, const int32_t *__restrict__ tab_,
                                                                    const uint32_t *__restrict__ ttab_, uint32_t max_bands, uint32_t n_images) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const uint32_t image = ((blockIdx.x >> 3) / max_bands) * 8u + (blockIdx.x & 7u), kind = image < n_images ? jobs[image].r.src_nc : 0u;  // (uniform)
    if (kind == 0u) resample_tensor_body<E, 0u>(jobs, tab_, ttab_, max_bands, n_images, lds_raw);
    else if (kind == 1u) resample_tensor_body<E, 1u>(jobs, tab_, ttab_, max_bands, n_images, lds_raw);
    else resample_tensor_body<E, 4u>(jobs, tab_, ttab_, max_bands, n_images, lds_raw);
}

hipError_t launch_resample_tensor(const TensorJob *d_jobs, const int32_t *d_tab, const void *d_ttab, uint32_t elem_bytes, uint32_t n_images, uint32_t max_bands,
                                  uint32_t lds_bytes, hipStream_t stream, bool rgb) {
    uint32_t wgs;
    hipError_t err;
    if (!band_grid(n_images, max_bands, lds_bytes, wgs, err)) return err;
    if (elem_bytes != 2u && elem_bytes != 4u) return hipErrorInvalidValue;
    const uint32_t lds = tensor_lds(lds_bytes, elem_bytes);
    const uint32_t *tt = (const uint32_t *)d_ttab;
    if (rgb && elem_bytes == 4u) resample_tensor_rgb_kernel<uint32_t><<<dim3(wgs), dim3(RS_NT), lds, stream>>>(d_jobs, d_tab, tt, max_bands, n_images);
    else if (rgb) resample_tensor_rgb_kernel<uint16_t><<<dim3(wgs), dim3(RS_NT), lds, stream>>>(d_jobs, d_tab, tt, max_bands, n_images);
    else if (elem_bytes == 4u) resample_tensor_kernel<uint32_t><<<dim3(wgs), dim3(RS_NT), lds, stream>>>(d_jobs, d_tab, tt, max_bands, n_images);
    else resample_tensor_kernel<uint16_t><<<dim3(wgs), dim3(RS_NT), lds, stream>>>(d_jobs, d_tab, tt, max_bands, n_images);
    return hipGetLastError();
}

// ---- Runs of bands: a workgroup takes the bands [band0, band1) of one image through run_walk (band_walk.hpp). ----
// The grid is the band kernels', numbered for the XCDs, over runs: image `image` takes XCD image % 8, its runs are consecutive slots.
__global__ __launch_bounds__(RS_NT, 4) void resample_run_kernel(const ResampleJob *__restrict__ jobs, const int32_t *__restrict__ tab_, const uint32_t *__restrict__ bprs,
                                                             uint32_t max_runs, uint32_t n_images) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, image = (slot / max_runs) * 8u + xcd, run = slot % max_runs;
    if (image >= n_images) return;
    const uint32_t bpr = bprs[image];
    if (bpr == 0u) return;  // (uniform: the image keeps its bands)
    const ResampleJob j = jobs[image];
    const uint32_t band0 = run * bpr, band1 = min(band0 + bpr, j.bands);
    if (band0 >= j.bands) return;  // (uniform)
    const JP_GLOBAL int32_t *tab = (const JP_GLOBAL int32_t *)tab_;
    DeviceLanes lanes;
    auto vstore = [&](uint32_t band, uint32_t tid) __attribute__((always_inline)) { RBand::vstore(j, tab, band, tid, lds_raw); };
    if (j.src_nc == 0u) run_walk<0u>(j, tab, band0, band1, lds_raw, vstore, lanes);  // (uniform; RGB output: the converting passes)
    else if (j.src_nc == 1u) run_walk<1u>(j, tab, band0, band1, lds_raw, vstore, lanes);
    else run_walk<4u>(j, tab, band0, band1, lds_raw, vstore, lanes);
}

template <class E>
__global__ __launch_bounds__(RS_NT, 4) void resample_tensor_run_kernel(const TensorJob *__restrict__ jobs, const int32_t *__restrict__ tab_,
                                                                    const uint32_t *__restrict__ ttab_, const uint32_t *__restrict__ bprs, uint32_t max_runs,
                                                                    uint32_t n_images) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, image = (slot / max_runs) * 8u + xcd, run = slot % max_runs;
    if (image >= n_images) return;
    const uint32_t bpr = bprs[image];
    if (bpr == 0u) return;  // (uniform)
    const TensorJob t = jobs[image];
    const uint32_t band0 = run * bpr, band1 = min(band0 + bpr, t.r.bands);
    if (band0 >= t.r.bands) return;  // (uniform)
    const JP_GLOBAL int32_t *tab = (const JP_GLOBAL int32_t *)tab_;
    TBand<E>::load_table(t, (const JP_GLOBAL uint32_t *)ttab_, threadIdx.x, lds_raw);  // (behind the rows: the move never reaches it)
    DeviceLanes lanes;
    auto vstore = [&](uint32_t band, uint32_t tid) __attribute__((always_inline)) { TBand<E>::vstore(t, tab, band, tid, lds_raw); };
    if (t.r.src_nc == 0u) run_walk<0u>(t.r, tab, band0, band1, lds_raw, vstore, lanes);
    else if (t.r.src_nc == 1u) run_walk<1u>(t.r, tab, band0, band1, lds_raw, vstore, lanes);
    else run_walk<4u>(t.r, tab, band0, band1, lds_raw, vstore, lanes);
}

hipError_t launch_resample_run(const ResampleJob *d_jobs, const int32_t *d_tab, const uint32_t *d_bpr, uint32_t n_images, uint32_t max_runs, uint32_t lds_bytes,
                               hipStream_t stream) {
    uint32_t wgs;
    hipError_t err;
    if (!band_grid(n_images, max_runs, lds_bytes, wgs, err)) return err;
    resample_run_kernel<<<dim3(wgs), dim3(RS_NT), lds_bytes, stream>>>(d_jobs, d_tab, d_bpr, max_runs, n_images);
    return hipGetLastError();
}

hipError_t launch_resample_tensor_run(const TensorJob *d_jobs, const int32_t *d_tab, const void *d_ttab, const uint32_t *d_bpr, uint32_t elem_bytes, uint32_t n_images,
                                      uint32_t max_runs, uint32_t lds_bytes, hipStream_t stream) {
    uint32_t wgs;
    hipError_t err;
    if (!band_grid(n_images, max_runs, lds_bytes, wgs, err)) return err;
    if (elem_bytes != 2u && elem_bytes != 4u) return hipErrorInvalidValue;
    const uint32_t lds = tensor_lds(lds_bytes, elem_bytes);
    const uint32_t *tt = (const uint32_t *)d_ttab;
    if (elem_bytes == 4u) resample_tensor_run_kernel<uint32_t><<<dim3(wgs), dim3(RS_NT), lds, stream>>>(d_jobs, d_tab, tt, d_bpr, max_runs, n_images);
    else resample_tensor_run_kernel<uint16_t><<<dim3(wgs), dim3(RS_NT), lds, stream>>>(d_jobs, d_tab, tt, d_bpr, max_runs, n_images);
    return hipGetLastError();
}

}  // namespace jpgpu
