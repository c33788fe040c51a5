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

// ---- Runs of bands: new kernels beside the band kernels above, which stay what they are. ----
// A workgroup owns the bands [band0, band1) of one image, every one of a single chunk.  The first band is the band kernels': horizontal
// pass of its source rows [s0, s1) into LDS rows 0.., barrier, vertical pass.  For every further band the rows it shares with the band
// before, [s0(b), s1(b - 1)), already lie in LDS: they move down to where this band expects them (row s - s0(b); RBand::roll_*: read,
// barrier, write, barrier per slab), and only the new rows [max(s1(b - 1), s0(b)), s1(b)) go through the horizontal pass.  The vertical
// pass (`vstore(band)`: RBand::vstore / TBand<E>::vstore) runs with the band index, unchanged.  LDS: the plan's lds_bytes, as ever.
template <uint32_t KIND, class V>
static __device__ __forceinline__ void resample_run_body(const ResampleJob &j, const JP_GLOBAL int32_t *tab, uint32_t band0, uint32_t band1, uint32_t tid,
                                                         uint8_t *lds, const V &vstore) {
    for (uint32_t band = band0; band < band1; band++) {  // (uniform)
        if (band == band0) {
            uint32_t r0, r1, s0, s1;
            RBand::rows_of(j, tab, band, r0, r1, s0, s1);
            RBand::hpass_rows_of<KIND>(j, tab, s0, s1 - s0, 0u, tid, lds);
        } else {
            uint32_t shift, keep, n0, s0, s1;
            RBand::roll_of(j, tab, band, shift, keep, n0, s0, s1);
            __syncthreads();  // (the vertical pass of the band before has read its rows)
            if (shift != 0u && keep != 0u) {
                const uint32_t slabs = RBand::roll_slabs(j, keep);
                for (uint32_t slab = 0; slab < slabs; slab++) {
                    uint32_t reg[RS_ROLL_DW];
                    RBand::roll_read(j, shift, keep, slab, tid, lds, reg);
                    __syncthreads();
                    RBand::roll_write(j, keep, slab, tid, lds, reg);
                    __syncthreads();
                }
            }
            if (s1 > n0) RBand::hpass_rows_of<KIND>(j, tab, n0, s1 - n0, n0 - s0, tid, lds);
        }
        __syncthreads();
        vstore(band);
    }
}

// The grid is the band kernels', numbered for the XCDs, over runs: image `image` takes XCD image % 8, its runs are consecutive slots.
__global__ __launch_bounds__(RS_NT, 4) void resample_run_kernel(const ResampleJob *__restrict__ jobs, const int32_t *__restrict__ tab_, const uint32_t *__restrict__ bprs,
                                                             uint32_t max_runs, uint32_t n_images) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, image = (slot / max_runs) * 8u + xcd, run = slot % max_runs;
    if (image >= n_images) return;
    const uint32_t bpr = bprs[image];
    if (bpr == 0u) return;  // (uniform: the image keeps its bands)
    const ResampleJob j = jobs[image];
    const uint32_t band0 = run * bpr, band1 = min(band0 + bpr, j.bands), tid = threadIdx.x;
    if (band0 >= j.bands) return;  // (uniform)
    const JP_GLOBAL int32_t *tab = (const JP_GLOBAL int32_t *)tab_;
    auto vstore = [&](uint32_t band) { RBand::vstore(j, tab, band, tid, lds_raw); };
    if (j.src_nc == 0u) resample_run_body<0u>(j, tab, band0, band1, tid, lds_raw, vstore);  // (uniform; RGB output: the converting passes)
    else if (j.src_nc == 1u) resample_run_body<1u>(j, tab, band0, band1, tid, lds_raw, vstore);
    else resample_run_body<4u>(j, tab, band0, band1, tid, lds_raw, vstore);
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
    const uint32_t band0 = run * bpr, band1 = min(band0 + bpr, t.r.bands), tid = threadIdx.x;
    if (band0 >= t.r.bands) return;  // (uniform)
    const JP_GLOBAL int32_t *tab = (const JP_GLOBAL int32_t *)tab_;
    TBand<E>::load_table(t, (const JP_GLOBAL uint32_t *)ttab_, tid, lds_raw);  // (behind the rows: the move never reaches it)
    auto vstore = [&](uint32_t band) { TBand<E>::vstore(t, tab, band, tid, lds_raw); };
    if (t.r.src_nc == 0u) resample_run_body<0u>(t.r, tab, band0, band1, tid, lds_raw, vstore);
    else if (t.r.src_nc == 1u) resample_run_body<1u>(t.r, tab, band0, band1, tid, lds_raw, vstore);
    else resample_run_body<4u>(t.r, tab, band0, band1, tid, lds_raw, vstore);
}

hipError_t launch_resample_run(const ResampleJob *d_jobs, const int32_t *d_tab, const uint32_t *d_bpr, uint32_t n_images, uint32_t max_runs, uint32_t lds_bytes,
                               hipStream_t stream) {
    if (n_images == 0 || max_runs == 0) return hipSuccess;
    if (lds_bytes > RS_MAX_LDS) return hipErrorInvalidValue;
    const uint64_t wgs = (((uint64_t)n_images + 7u) / 8u) * 8u * max_runs;
    if (wgs > 0x7fffffffull) return hipErrorInvalidValue;
    resample_run_kernel<<<dim3((uint32_t)wgs), dim3(RS_NT), lds_bytes, stream>>>(d_jobs, d_tab, d_bpr, max_runs, n_images);
    return hipGetLastError();
}

hipError_t launch_resample_tensor_run(const TensorJob *d_jobs, const int32_t *d_tab, const void *d_ttab, const uint32_t *d_bpr, uint32_t elem_bytes, uint32_t n_images,
                                      uint32_t max_runs, uint32_t lds_bytes, hipStream_t stream) {
    if (n_images == 0 || max_runs == 0) return hipSuccess;
    if (lds_bytes > RS_MAX_LDS || (elem_bytes != 2u && elem_bytes != 4u)) return hipErrorInvalidValue;
    const uint64_t wgs = (((uint64_t)n_images + 7u) / 8u) * 8u * max_runs;
    if (wgs > 0x7fffffffull) return hipErrorInvalidValue;
    const uint32_t lds = ((lds_bytes + 15u) & ~15u) + 4u * 256u * elem_bytes;  // the rows, then the table
    if (elem_bytes == 4u)
        resample_tensor_run_kernel<uint32_t><<<dim3((uint32_t)wgs), dim3(RS_NT), lds, stream>>>(d_jobs, d_tab, (const uint32_t *)d_ttab, d_bpr, max_runs, n_images);
    else
        resample_tensor_run_kernel<uint16_t><<<dim3((uint32_t)wgs), dim3(RS_NT), lds, stream>>>(d_jobs, d_tab, (const uint32_t *)d_ttab, d_bpr, max_runs, n_images);
    return hipGetLastError();
}

}  // namespace jpgpu
