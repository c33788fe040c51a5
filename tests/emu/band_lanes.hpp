// band_lanes.hpp — TEST-ONLY: the lanes policy under which the CPU emulation runs the product's walks (csrc/band_walk.hpp), and the
// launches of csrc/resample.hip and csrc/placed.hip workgroup by workgroup: the kernels' prologues, then band_walk / run_walk.
//
// HostLanes holds the phases a walk issues and runs them at the next barrier, lane by lane: lane 0 runs every phase since the barrier
// before, then lane 1, and so on — what a workgroup may do between two barriers.  A lane that reads LDS another lane has yet to write
// reads the 0xCD poison (rows_dead; fresh LDS is poisoned too), so a barrier that band_walk.hpp lacks or misplaces changes the bytes.
#pragma once
#include <functional>
#include <vector>

#include "../../jpeg-decoder_amd/csrc/band_walk.hpp"

namespace jpgpu {

struct HostLanes {
    template <uint32_t N>
    struct Sums {
        std::vector<int32_t> v = std::vector<int32_t>(RS_NT * N);
        int32_t (&of(uint32_t tid))[N] { return *reinterpret_cast<int32_t(*)[N]>(&v[N * tid]); }
    };
    struct Regs {
        std::vector<uint32_t> v = std::vector<uint32_t>(RS_NT * RS_ROLL_DW);
        uint32_t (&of(uint32_t tid))[RS_ROLL_DW] { return *reinterpret_cast<uint32_t(*)[RS_ROLL_DW]>(&v[RS_ROLL_DW * tid]); }
    };
    std::vector<std::function<void(uint32_t)>> phases;
    template <class F>
    void each(const F &f) {
        phases.emplace_back(f);
    }
    void barrier() {
        for (uint32_t tid = 0; tid < RS_NT; tid++)
            for (auto &f : phases) f(tid);
        phases.clear();
    }
    void rows_dead(uint8_t *rows, uint32_t bytes) { memset(rows, 0xCD, bytes); }
    void done() { barrier(); }  // (the lanes run to the kernel's end)
};

// LDS of a workgroup: `bytes` at a 16-byte boundary
struct HostLds {
    std::vector<uint8_t> store;
    uint8_t *p;
    uint32_t bytes;
    explicit HostLds(uint32_t n) : store(n + 16), p(store.data() + ((16 - ((uintptr_t)store.data() & 15)) & 15)), bytes(n) {}
    void fresh() { memset(p, 0xCD, bytes); }  // garbage, like real LDS
};
inline uint32_t host_tensor_lds(const ResampleJob &j) { return ((j.lds_bytes + 15u) & ~15u) + TN_TABLE_MAX; }

// the kernels' dispatch on the job's src_nc: 0 -> the job's channels, 1 -> gray, anything else -> CMYK
template <uint32_t K>
struct Kind {
    static constexpr uint32_t value = K;
};
template <class F>
void with_kind(uint32_t src_nc, const F &f) {
    if (src_nc == 0u) f(Kind<0u>());
    else if (src_nc == 1u) f(Kind<1u>());
    else f(Kind<4u>());
}
// one workgroup's band, its chunks counted
template <class B>
void walk_band(const B &band, HostLanes &lanes, uint32_t &most) {
    most = max(most, band.chunks());
    band_walk(band, lanes);
}

// resample_band_kernel / resample_band_rgb_kernel.  most: the most chunks of a band
inline void emu_launch_u8(const ResampleJob &j, const int32_t *tab, uint32_t &most) {
    HostLds lds(j.lds_bytes);
    for (uint32_t band = 0; band < j.bands; band++) {
        lds.fresh();
        HostLanes lanes;
        with_kind(j.src_nc, [&](auto k) { walk_band(U8Band<decltype(k)::value>(j, tab, band, lds.p), lanes, most); });
    }
}
// resample_tensor_kernel / resample_tensor_rgb_kernel
template <class E>
void emu_launch_tensor(const TensorJob &t, const int32_t *tab, const uint32_t *ttab, uint32_t &most) {
    HostLds lds(host_tensor_lds(t.r));
    for (uint32_t band = 0; band < t.r.bands; band++) {
        lds.fresh();
        HostLanes lanes;
        lanes.each([&](uint32_t tid) { TBand<E>::load_table(t, ttab, tid, lds.p); });
        with_kind(t.r.src_nc, [&](auto k) { walk_band(TensorBand<E, decltype(k)::value>(t, tab, band, lds.p), lanes, most); });
    }
}
// resample_placed_kernel / resample_placed_rgb_kernel.  fill_bands: bands without a visible row
inline void emu_launch_placed(const PlacedJob &pj, const int32_t *tab, uint32_t &most, uint32_t &fill_bands) {
    const ResampleJob &j = pj.r;
    HostLds lds(j.lds_bytes);
    for (uint32_t band = 0; band < pj.p.bands; band++) {
        uint32_t R0, R1, ib;
        bool vis;
        PBand::band_of(j, pj.p, band, R0, R1, ib, vis);
        lds.fresh();
        HostLanes lanes;
        if (!vis) {
            fill_bands++;
            lanes.each([&](uint32_t tid) { PBand::fill_band(j, pj.p, band, tid); });
            lanes.done();
            continue;
        }
        with_kind(j.src_nc, [&](auto k) { walk_band(PlacedBand<decltype(k)::value>(j, &pj, tab, band, ib, pj.p.shift, lds.p), lanes, most); });
    }
}
// resample_placed_tensor_kernel / resample_placed_tensor_rgb_kernel
template <class E>
void emu_launch_placed_tensor(const PlacedTensorJob &t, const int32_t *tab, const uint32_t *ttab, uint32_t &most, uint32_t &fill_bands) {
    const ResampleJob &j = t.t.r;
    HostLds lds(host_tensor_lds(j));
    for (uint32_t band = 0; band < t.p.bands; band++) {
        uint32_t R0, R1, ib;
        bool vis;
        PBand::band_of(j, t.p, band, R0, R1, ib, vis);
        lds.fresh();
        HostLanes lanes;
        lanes.each([&](uint32_t tid) { TBand<E>::load_table(t.t, ttab, tid, lds.p); });
        if (!vis) {
            fill_bands++;
            lanes.barrier();
            lanes.rows_dead(lds.p, j.lds_bytes);  // (a band of fill reads no LDS row)
            lanes.each([&](uint32_t tid) { PTBand<E>::fill_band(t, band, tid, lds.p); });
            lanes.done();
            continue;
        }
        with_kind(j.src_nc, [&](auto k) { walk_band(PlacedTensorBand<E, decltype(k)::value>(t, tab, band, ib, lds.p), lanes, most); });
    }
}

}  // namespace jpgpu
