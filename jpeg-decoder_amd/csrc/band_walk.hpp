// band_walk.hpp — the walk of a band through LDS, stated once: the band kernels of resample.hip and placed.hip run it (all but
// resample_tensor_kernel, which has it written out), and so does the CPU emulation of tests/emu.
//
//   band_walk   one chunk:   horizontal pass into LDS | barrier | vertical pass and store
//               more:        per group of RS_NT destination items the sums are zeroed; per chunk  barrier | horizontal pass | barrier |
//                            accumulate;  behind the last chunk the sums are put.  Nothing waits behind the last store.
//   run_walk    a run of one-chunk bands whose shared source rows stay in LDS.
//
// Two policies.  A BAND policy holds the job, the tables, the band and the LDS pointer and answers chunks(), width(), hpass(chunk, x0,
// x1, tid), vstore(tid), groups(), group_columns(group, x0, x1), vacc(chunk, group, tid, sum), vput(group, tid, sum), NSUM: the phase
// bodies of RBand / TBand / PBand / PTBand under one set of names (U8Band, TensorBand, PlacedBand, PlacedTensorBand below; KIND: the
// horizontal pass, as RBand::hpass_of).  A LANES policy says how a workgroup's lanes run a phase: each(f) runs f(tid) for the lanes,
// barrier() is the workgroup barrier, Sums<N> / Regs are a lane's registers.  On the device (DeviceLanes, below) a lane is a thread; in
// tests/emu a phase runs for the RS_NT lanes in turn and the barriers decide what a lane has seen of the others.  rows_dead(p, n) tells
// the lanes policy that the n bytes of LDS rows at p hold nothing any more (the next horizontal pass overwrites them) and done() that
// the workgroup has issued its last phase: both are empty on the device, the emulation poisons the rows and runs what it still holds.
// A phase's lambda takes what it needs by value (an emulated phase runs at the next barrier), the lane's registers by reference.
#pragma once
#include "placed_band.hpp"

namespace jpgpu {

#ifdef JPGPU_RS_DEVICE_BODY
// What the four band policies share: the resample job, its tables, its band `ib` and the LDS rows, which begin `shift` bytes into LDS.
template <uint32_t KIND>
struct BandRows {
    const ResampleJob &j;
    const JP_GLOBAL int32_t *tab;
    uint32_t ib;
    uint8_t *lds;
    uint32_t shift;
    __device__ __forceinline__ uint32_t chunks() const { return RBand::chunks_of(j, tab, ib); }
    __device__ __forceinline__ uint32_t width() const { return j.out_w; }
    __device__ __forceinline__ void hpass(uint32_t chunk, uint32_t x0, uint32_t x1, uint32_t tid) const {
        RBand::hpass_of<KIND>(j, tab, ib, chunk, x0, x1, tid, lds + shift);
    }
};

template <uint32_t KIND>
struct U8Band : BandRows<KIND> {
    static constexpr uint32_t NSUM = 4;
    using BandRows<KIND>::j, BandRows<KIND>::tab, BandRows<KIND>::ib, BandRows<KIND>::lds;
    __device__ __forceinline__ U8Band(const ResampleJob &j_, const JP_GLOBAL int32_t *tab_, uint32_t band, uint8_t *lds_) : BandRows<KIND>{j_, tab_, band, lds_, 0u} {}
    __device__ __forceinline__ void vstore(uint32_t tid) const { RBand::vstore(j, tab, ib, tid, lds); }
    __device__ __forceinline__ uint32_t groups() const { return RBand::groups_of(j, ib); }
    __device__ __forceinline__ void group_columns(uint32_t group, uint32_t &x0, uint32_t &x1) const { RBand::group_columns(j, ib, group, x0, x1); }
    __device__ __forceinline__ void vacc(uint32_t chunk, uint32_t group, uint32_t tid, int32_t (&sum)[4]) const { RBand::vacc(j, tab, ib, chunk, group, tid, lds, sum); }
    __device__ __forceinline__ void vput(uint32_t group, uint32_t tid, const int32_t (&sum)[4]) const { RBand::vput(j, ib, group, tid, sum); }
};

template <class E, uint32_t KIND>
struct TensorBand : BandRows<KIND> {
    static constexpr uint32_t NSUM = 16;
    using BandRows<KIND>::tab, BandRows<KIND>::ib, BandRows<KIND>::lds;
    const TensorJob &t;
    __device__ __forceinline__ TensorBand(const TensorJob &t_, const JP_GLOBAL int32_t *tab_, uint32_t band, uint8_t *lds_)
        : BandRows<KIND>{t_.r, tab_, band, lds_, 0u}, t(t_) {}
    __device__ __forceinline__ void vstore(uint32_t tid) const { TBand<E>::vstore(t, tab, ib, tid, lds); }
    __device__ __forceinline__ uint32_t groups() const { return TBand<E>::groups_of(t, ib); }
    __device__ __forceinline__ void group_columns(uint32_t group, uint32_t &x0, uint32_t &x1) const { TBand<E>::group_columns(t, ib, group, x0, x1); }
    __device__ __forceinline__ void vacc(uint32_t chunk, uint32_t group, uint32_t tid, int32_t (&sum)[16]) const {
        TBand<E>::vacc(t, tab, ib, chunk, group, tid, lds, sum);
    }
    __device__ __forceinline__ void vput(uint32_t group, uint32_t tid, const int32_t (&sum)[16]) const { TBand<E>::vput(t, ib, group, tid, sum, lds); }
};

// The job's placement, loaded where it is used: the compiler does not carry it from an earlier load.
static __device__ __forceinline__ Place place_again(const PlacedJob *jp) {
#ifndef JPGPU_HOST_EMULATION
    asm volatile("" : "+s"(jp));
#endif
    return jp->p;
}

// `band`: the canvas band, `ib` the band of the visible rectangle's job whose rows lie in it (PBand::band_of).  The placement is read
// again behind every horizontal pass: kept in registers across it, the kernel spills.
template <uint32_t KIND>
struct PlacedBand : BandRows<KIND> {
    static constexpr uint32_t NSUM = 4;
    using BandRows<KIND>::j, BandRows<KIND>::tab, BandRows<KIND>::ib, BandRows<KIND>::lds;
    const PlacedJob *jp;
    uint32_t band;
    __device__ __forceinline__ PlacedBand(const ResampleJob &j_, const PlacedJob *jp_, const JP_GLOBAL int32_t *tab_, uint32_t band_, uint32_t ib_, uint32_t shift_,
                                          uint8_t *lds_)
        : BandRows<KIND>{j_, tab_, ib_, lds_, shift_}, jp(jp_), band(band_) {}
    __device__ __forceinline__ void vstore(uint32_t tid) const { PBand::vstore(j, place_again(jp), tab, band, ib, tid, lds); }
    __device__ __forceinline__ uint32_t groups() const { return PBand::groups_of(j, place_again(jp), band); }
    __device__ __forceinline__ void group_columns(uint32_t group, uint32_t &x0, uint32_t &x1) const {
        PBand::group_columns(j, place_again(jp), band, group, x0, x1);
    }
    __device__ __forceinline__ void vacc(uint32_t chunk, uint32_t group, uint32_t tid, int32_t (&sum)[4]) const {
        PBand::vacc(j, place_again(jp), tab, band, ib, chunk, group, tid, lds, sum);
    }
    __device__ __forceinline__ void vput(uint32_t group, uint32_t tid, const int32_t (&sum)[4]) const { PBand::vput(j, place_again(jp), band, group, tid, sum); }
};

template <class E, uint32_t KIND>
struct PlacedTensorBand : BandRows<KIND> {
    static constexpr uint32_t NSUM = 16;
    using BandRows<KIND>::tab, BandRows<KIND>::ib, BandRows<KIND>::lds;
    const PlacedTensorJob &t;
    uint32_t band;
    __device__ __forceinline__ PlacedTensorBand(const PlacedTensorJob &t_, const JP_GLOBAL int32_t *tab_, uint32_t band_, uint32_t ib_, uint8_t *lds_)
        : BandRows<KIND>{t_.t.r, tab_, ib_, lds_, t_.p.shift}, t(t_), band(band_) {}
    __device__ __forceinline__ void vstore(uint32_t tid) const { PTBand<E>::vstore(t, tab, band, ib, tid, lds); }
    __device__ __forceinline__ uint32_t groups() const { return PTBand<E>::groups_of(t, band); }
    __device__ __forceinline__ void group_columns(uint32_t group, uint32_t &x0, uint32_t &x1) const { PTBand<E>::group_columns(t, band, group, x0, x1); }
    __device__ __forceinline__ void vacc(uint32_t chunk, uint32_t group, uint32_t tid, int32_t (&sum)[16]) const {
        PTBand<E>::vacc(t, tab, band, ib, chunk, group, tid, lds, sum);
    }
    __device__ __forceinline__ void vput(uint32_t group, uint32_t tid, const int32_t (&sum)[16]) const { PTBand<E>::vput(t, band, group, tid, sum, lds); }
};

template <class B, class L>
static __device__ __forceinline__ void band_walk(const B &band, L &lanes) {
    const uint32_t chunks = band.chunks();
    if (chunks == 1u) {  // (uniform) the band's source rows fit: one horizontal pass, every item summed and stored
        lanes.each([=](uint32_t tid) __attribute__((always_inline)) { band.hpass(0u, 0u, band.width(), tid); });
        lanes.barrier();
        lanes.each([=](uint32_t tid) __attribute__((always_inline)) { band.vstore(tid); });
        lanes.done();
        return;
    }
    const uint32_t groups = band.groups();
    typename L::template Sums<B::NSUM> sums;
    for (uint32_t group = 0; group < groups; group++) {
        uint32_t x0, x1;
        band.group_columns(group, x0, x1);
        lanes.each([&sums](uint32_t tid) __attribute__((always_inline)) {
#pragma unroll
            for (uint32_t i = 0; i < B::NSUM; i++) sums.of(tid)[i] = 0;
        });
        for (uint32_t chunk = 0; chunk < chunks; chunk++) {
            lanes.barrier();  // (the vertical pass before has read its rows; a tensor's table is in place)
            lanes.rows_dead(band.lds, band.j.lds_bytes);
            lanes.each([=](uint32_t tid) __attribute__((always_inline)) { band.hpass(chunk, x0, x1, tid); });
            lanes.barrier();
            lanes.each([=, &sums](uint32_t tid) __attribute__((always_inline)) { band.vacc(chunk, group, tid, sums.of(tid)); });
        }
        lanes.each([=, &sums](uint32_t tid) __attribute__((always_inline)) { band.vput(group, tid, sums.of(tid)); });
    }
    lanes.done();
}

// The move of a run's kept rows down by `shift` rows (RBand::roll_*): per slab every lane reads, barrier, writes, barrier.
template <class L>
static __device__ __forceinline__ void roll_move(const ResampleJob &j, uint32_t shift, uint32_t keep, uint8_t *lds, L &lanes) {
    const uint32_t slabs = RBand::roll_slabs(j, keep);
    typename L::Regs reg;
    for (uint32_t slab = 0; slab < slabs; slab++) {
        lanes.each([=, &j, &reg](uint32_t tid) __attribute__((always_inline)) { RBand::roll_read(j, shift, keep, slab, tid, lds, reg.of(tid)); });
        lanes.barrier();
        lanes.each([=, &j, &reg](uint32_t tid) __attribute__((always_inline)) { RBand::roll_write(j, keep, slab, tid, lds, reg.of(tid)); });
        lanes.barrier();
    }
}

// A workgroup owns the bands [band0, band1) of one image, every one of a single chunk.  The first band is the band kernels': horizontal
// pass of its source rows [s0, s1) into LDS rows 0.., barrier, vertical pass.  For every further band the rows it shares with the band
// before, [s0(b), s1(b - 1)), already lie in LDS: they move down to where this band expects them (row s - s0(b)), and only the new rows
// [max(s1(b - 1), s0(b)), s1(b)) go through the horizontal pass.  The vertical pass (`vstore(band, tid)`: RBand::vstore /
// TBand<E>::vstore) runs with the band index, unchanged.  LDS: the plan's lds_bytes, as ever.
template <uint32_t KIND, class V, class L>
static __device__ __forceinline__ void run_walk(const ResampleJob &j, const JP_GLOBAL int32_t *tab, uint32_t band0, uint32_t band1, uint8_t *lds, const V &vstore,
                                                L &lanes) {
    for (uint32_t band = band0; band < band1; band++) {  // (uniform)
        if (band == band0) {
            uint32_t r0, r1, s0, s1;
            RBand::rows_of(j, tab, band, r0, r1, s0, s1);
            lanes.each([=, &j](uint32_t tid) __attribute__((always_inline)) { RBand::hpass_rows_of<KIND>(j, tab, s0, s1 - s0, 0u, tid, lds); });
        } else {
            uint32_t shift, keep, n0, s0, s1;
            RBand::roll_of(j, tab, band, shift, keep, n0, s0, s1);
            lanes.barrier();  // (the vertical pass of the band before has read its rows)
            if (shift != 0u && keep != 0u) roll_move(j, shift, keep, lds, lanes);
            if (keep < s1 - s0) lanes.rows_dead(lds + keep * j.pitch, (s1 - s0 - keep) * j.pitch);
            if (s1 > n0) lanes.each([=, &j](uint32_t tid) __attribute__((always_inline)) { RBand::hpass_rows_of<KIND>(j, tab, n0, s1 - n0, n0 - s0, tid, lds); });
        }
        lanes.barrier();
        lanes.each([=](uint32_t tid) __attribute__((always_inline)) { vstore(band, tid); });
    }
    lanes.done();
}
#endif  // JPGPU_RS_DEVICE_BODY

}  // namespace jpgpu

#if defined(__HIP__) && !defined(JPGPU_HOST_EMULATION)
namespace jpgpu {
// The lanes of a workgroup on the device: a lane is a thread, its sums and registers are its own.
struct DeviceLanes {
    template <uint32_t N>
    struct Sums {
        int32_t v[N];
        __device__ __forceinline__ int32_t (&of(uint32_t))[N] { return v; }
    };
    struct Regs {
        uint32_t v[RS_ROLL_DW];
        __device__ __forceinline__ uint32_t (&of(uint32_t))[RS_ROLL_DW] { return v; }
    };
    template <class F>
    __device__ __forceinline__ void each(const F &f) const {
        f(threadIdx.x);
    }
    __device__ __forceinline__ void barrier() const { __syncthreads(); }
    __device__ __forceinline__ void rows_dead(const uint8_t *, uint32_t) const {}
    __device__ __forceinline__ void done() const {}
};

// The grid of the band kernels (8 XCDs x images x `per_image` bands or runs, resample.hip) and what every launcher checks before it:
// false with `err` set where nothing is launched — an empty launch (hipSuccess), more LDS than a workgroup has, a grid beyond 2^31.
inline bool band_grid(uint32_t n_images, uint32_t per_image, uint32_t lds_bytes, uint32_t &wgs, hipError_t &err) {
    err = hipSuccess;
    if (n_images == 0 || per_image == 0) return false;
    err = hipErrorInvalidValue;
    const uint64_t n = (((uint64_t)n_images + 7u) / 8u) * 8u * per_image;
    if (lds_bytes > RS_MAX_LDS || n > 0x7fffffffull) return false;
    wgs = (uint32_t)n;
    return true;
}
// LDS of a tensor kernel: the rows, then the table
inline uint32_t tensor_lds(uint32_t lds_bytes, uint32_t elem_bytes) { return ((lds_bytes + 15u) & ~15u) + 4u * 256u * elem_bytes; }
}  // namespace jpgpu
#endif
