// emu_filters.cpp — TEST-ONLY CPU emulation of the band kernels (csrc/resample.hip, csrc/placed.hip) under the filters of DESIGN.md
// §4.15: the product's filtered tables, its planners and every workgroup of the launch grid, lane by lane and phase by phase (the
// kernels' barriers are the phase boundaries).  The kernels do not know the filter: they get wider tables with negative weights.
// And the run kernels (resample_run_body): the workgroups of the runs of bands, the move of the kept rows in its read and write phases.
// Built by tests/test_filters_emulation.py (g++, the flags of tests/emu/Makefile).
#include "hip_shim.hpp"
#include <vector>
#include "../../jpeg-decoder_amd/csrc/placed_band.hpp"

using namespace jpgpu;

namespace {

struct Geometry {
    uint32_t filter, in_w, in_h, nc, kind;  // kind 1 / 4: a gray / CMYK source converted to three channels (nc is 1 / 4 then)
    uint32_t cw, ch;                        // the output size
    uint32_t placed;                        // 0: the resample to cw x ch (resample.hip); 1: the placed kernels with (rw, rh, x, y)
    uint32_t rw, rh;
    int32_t x, y;
    uint32_t lds_cap, rb_cap;
};

// tables of the (visible) ranges under the filter, and the plan.  0, -1 planner refusal, -3 nothing visible
int plan(const Geometry &g, ResampleJob &j, Place &p, std::vector<int32_t> &tab, const uint8_t *fill) {
    uint32_t fx = 0, fy = 0;
    const uint32_t rw = g.placed ? g.rw : g.cw, rh = g.placed ? g.rh : g.ch;
    j.in_w = g.in_w, j.in_h = g.in_h, j.nc = g.kind ? 3u : g.nc, j.src_nc = g.kind;
    j.out_w = g.cw, j.out_h = g.ch;
    if (g.placed) {
        if (!placed_axis(rw, g.x, g.cw, fx, j.out_w, p.vx) || !placed_axis(rh, g.y, g.ch, fy, j.out_h, p.vy)) return -3;
        p.cw = g.cw, p.ch = g.ch;
        p.fill = (uint32_t)fill[0] | ((uint32_t)fill[1] << 8) | ((uint32_t)fill[2] << 16) | ((uint32_t)fill[3] << 24);
    }
    j.hks = resample_ksize_filtered(g.filter, g.in_w, rw), j.vks = resample_ksize_filtered(g.filter, g.in_h, rh);
    j.hb = 0, j.hk = j.hb + 2u * j.out_w, j.vb = j.hk + j.out_w * j.hks, j.vk = j.vb + 2u * j.out_h;
    tab.assign((size_t)j.vk + (size_t)j.out_h * j.vks, 0);
    resample_coefficients_range_filtered(g.filter, g.in_w, rw, fx, j.out_w, tab.data() + j.hb, tab.data() + j.hk, j.hks);
    resample_coefficients_range_filtered(g.filter, g.in_h, rh, fy, j.out_h, tab.data() + j.vb, tab.data() + j.vk, j.vks);
    if (g.placed) return placed_plan(j, p, tab.data(), g.lds_cap, g.rb_cap) ? 0 : -1;
    return resample_plan(j, tab.data(), g.lds_cap, g.rb_cap) ? 0 : -1;
}

void hpass_kind(const ResampleJob &j, const int32_t *tab, uint32_t ib, uint32_t chunk, uint32_t x0, uint32_t x1, uint32_t tid, uint8_t *rows) {
    if (j.src_nc == 1u) RBand::hpass_of<1u>(j, tab, ib, chunk, x0, x1, tid, rows);
    else if (j.src_nc == 4u) RBand::hpass_of<4u>(j, tab, ib, chunk, x0, x1, tid, rows);
    else RBand::hpass_of<0u>(j, tab, ib, chunk, x0, x1, tid, rows);
}

void hpass_rows_kind(const ResampleJob &j, const int32_t *tab, uint32_t c0, uint32_t nrows, uint32_t l0, uint32_t tid, uint8_t *rows) {
    if (j.src_nc == 1u) RBand::hpass_rows_of<1u>(j, tab, c0, nrows, l0, tid, rows);
    else if (j.src_nc == 4u) RBand::hpass_rows_of<4u>(j, tab, c0, nrows, l0, tid, rows);
    else RBand::hpass_rows_of<0u>(j, tab, c0, nrows, l0, tid, rows);
}

// info: rb, the job's bands, cap_rows, most chunks of a band, lds_bytes, launch bands, hks, vks, whether a weight of the horizontal /
// the vertical table is negative
void fill_info(uint32_t *info, const ResampleJob &j, const std::vector<int32_t> &tab, uint32_t bands, uint32_t most) {
    if (!info) return;
    info[0] = j.rb, info[1] = j.bands, info[2] = j.cap_rows, info[3] = most, info[4] = j.lds_bytes, info[5] = bands, info[6] = j.hks, info[7] = j.vks;
    info[8] = info[9] = 0;
    for (size_t i = j.hk; i < j.vb; i++) info[8] |= tab[i] < 0;
    for (size_t i = j.vk; i < tab.size(); i++) info[9] |= tab[i] < 0;
}

// resample_band_kernel / resample_band_rgb_kernel
void run_u8(const ResampleJob &j, const int32_t *tab, uint8_t *lds, uint32_t &most) {
    typedef int32_t Sum[4];
    std::vector<int32_t> acc(RS_NT * 4);
    for (uint32_t band = 0; band < j.bands; band++) {
        const uint32_t chunks = RBand::chunks_of(j, tab, band);
        most = chunks > most ? chunks : most;
        memset(lds, 0xCD, j.lds_bytes);  // garbage, like real LDS
        if (chunks == 1u) {
            for (uint32_t t = 0; t < RS_NT; t++) hpass_kind(j, tab, band, 0u, 0u, j.out_w, t, lds);
            for (uint32_t t = 0; t < RS_NT; t++) RBand::vstore(j, tab, band, t, lds);
            continue;
        }
        const uint32_t groups = RBand::groups_of(j, band);
        for (uint32_t group = 0; group < groups; group++) {
            uint32_t x0, x1;
            RBand::group_columns(j, band, group, x0, x1);
            std::fill(acc.begin(), acc.end(), 0);
            for (uint32_t chunk = 0; chunk < chunks; chunk++) {
                memset(lds, 0xCD, j.lds_bytes);
                for (uint32_t t = 0; t < RS_NT; t++) hpass_kind(j, tab, band, chunk, x0, x1, t, lds);
                for (uint32_t t = 0; t < RS_NT; t++) RBand::vacc(j, tab, band, chunk, group, t, lds, *reinterpret_cast<Sum *>(&acc[4 * t]));
            }
            for (uint32_t t = 0; t < RS_NT; t++) RBand::vput(j, band, group, t, *reinterpret_cast<Sum *>(&acc[4 * t]));
        }
    }
}

// placed_band_kernel and its RGB instance
void run_placed_u8(const PlacedJob &pj, const int32_t *tab, uint8_t *lds, uint32_t &most) {
    typedef int32_t Sum[4];
    std::vector<int32_t> acc(RS_NT * 4);
    const ResampleJob &j = pj.r;
    for (uint32_t band = 0; band < pj.p.bands; band++) {
        uint32_t R0, R1, ib;
        bool vis;
        PBand::band_of(j, pj.p, band, R0, R1, ib, vis);
        memset(lds, 0xCD, j.lds_bytes);
        if (!vis) {
            for (uint32_t tid = 0; tid < RS_NT; tid++) PBand::fill_band(j, pj.p, band, tid);
            continue;
        }
        uint8_t *rows = lds + pj.p.shift;
        const uint32_t chunks = RBand::chunks_of(j, tab, ib);
        most = chunks > most ? chunks : most;
        if (chunks == 1u) {
            for (uint32_t tid = 0; tid < RS_NT; tid++) hpass_kind(j, tab, ib, 0u, 0u, j.out_w, tid, rows);
            for (uint32_t tid = 0; tid < RS_NT; tid++) PBand::vstore(j, pj.p, tab, band, ib, tid, lds);
            continue;
        }
        const uint32_t groups = PBand::groups_of(j, pj.p, band);
        for (uint32_t group = 0; group < groups; group++) {
            uint32_t x0, x1;
            PBand::group_columns(j, pj.p, band, group, x0, x1);
            std::fill(acc.begin(), acc.end(), 0);
            for (uint32_t chunk = 0; chunk < chunks; chunk++) {
                memset(lds, 0xCD, j.lds_bytes);
                for (uint32_t tid = 0; tid < RS_NT; tid++) hpass_kind(j, tab, ib, chunk, x0, x1, tid, rows);
                for (uint32_t tid = 0; tid < RS_NT; tid++) PBand::vacc(j, pj.p, tab, band, ib, chunk, group, tid, lds, *reinterpret_cast<Sum *>(&acc[4 * tid]));
            }
            for (uint32_t tid = 0; tid < RS_NT; tid++) PBand::vput(j, pj.p, band, group, tid, *reinterpret_cast<Sum *>(&acc[4 * tid]));
        }
    }
}

// resample_tensor_kernel / resample_tensor_rgb_kernel
template <class E>
void run_tensor(const TensorJob &t, const int32_t *tab, const uint32_t *ttab, uint8_t *lds, uint32_t lds_total, uint32_t &most) {
    typedef int32_t Sum[16];
    std::vector<int32_t> acc(RS_NT * 16);
    const ResampleJob &j = t.r;
    for (uint32_t band = 0; band < j.bands; band++) {
        const uint32_t chunks = RBand::chunks_of(j, tab, band);
        most = chunks > most ? chunks : most;
        memset(lds, 0xCD, lds_total);
        for (uint32_t tid = 0; tid < RS_NT; tid++) TBand<E>::load_table(t, ttab, tid, lds);
        if (chunks == 1u) {
            for (uint32_t tid = 0; tid < RS_NT; tid++) hpass_kind(j, tab, band, 0u, 0u, j.out_w, tid, lds);
            for (uint32_t tid = 0; tid < RS_NT; tid++) TBand<E>::vstore(t, tab, band, tid, lds);
            continue;
        }
        const uint32_t groups = TBand<E>::groups_of(t, band);
        for (uint32_t group = 0; group < groups; group++) {
            uint32_t x0, x1;
            TBand<E>::group_columns(t, band, group, x0, x1);
            std::fill(acc.begin(), acc.end(), 0);
            for (uint32_t chunk = 0; chunk < chunks; chunk++) {
                memset(lds, 0xCD, j.lds_bytes);  // (the rows only: the table stays)
                for (uint32_t tid = 0; tid < RS_NT; tid++) hpass_kind(j, tab, band, chunk, x0, x1, tid, lds);
                for (uint32_t tid = 0; tid < RS_NT; tid++) TBand<E>::vacc(t, tab, band, chunk, group, tid, lds, *reinterpret_cast<Sum *>(&acc[16 * tid]));
            }
            for (uint32_t tid = 0; tid < RS_NT; tid++) TBand<E>::vput(t, band, group, tid, *reinterpret_cast<Sum *>(&acc[16 * tid]), lds);
        }
    }
}

// placed_tensor_kernel and its RGB instance
template <class E>
void run_placed_tensor(const PlacedTensorJob &t, const int32_t *tab, const uint32_t *ttab, uint8_t *lds, uint32_t lds_total, uint32_t &most) {
    typedef int32_t Sum[16];
    std::vector<int32_t> acc(RS_NT * 16);
    const ResampleJob &j = t.t.r;
    for (uint32_t band = 0; band < t.p.bands; band++) {
        uint32_t R0, R1, ib;
        bool vis;
        PBand::band_of(j, t.p, band, R0, R1, ib, vis);
        memset(lds, 0xCD, lds_total);
        for (uint32_t tid = 0; tid < RS_NT; tid++) TBand<E>::load_table(t.t, ttab, tid, lds);
        if (!vis) {
            memset(lds, 0xCD, j.lds_bytes);  // (a band of fill reads no LDS row)
            for (uint32_t tid = 0; tid < RS_NT; tid++) PTBand<E>::fill_band(t, band, tid, lds);
            continue;
        }
        uint8_t *rows = lds + t.p.shift;
        const uint32_t chunks = RBand::chunks_of(j, tab, ib);
        most = chunks > most ? chunks : most;
        if (chunks == 1u) {
            for (uint32_t tid = 0; tid < RS_NT; tid++) hpass_kind(j, tab, ib, 0u, 0u, j.out_w, tid, rows);
            for (uint32_t tid = 0; tid < RS_NT; tid++) PTBand<E>::vstore(t, tab, band, ib, tid, lds);
            continue;
        }
        const uint32_t groups = PTBand<E>::groups_of(t, band);
        for (uint32_t group = 0; group < groups; group++) {
            uint32_t x0, x1;
            PTBand<E>::group_columns(t, band, group, x0, x1);
            std::fill(acc.begin(), acc.end(), 0);
            for (uint32_t chunk = 0; chunk < chunks; chunk++) {
                memset(lds, 0xCD, j.lds_bytes);
                for (uint32_t tid = 0; tid < RS_NT; tid++) hpass_kind(j, tab, ib, chunk, x0, x1, tid, rows);
                for (uint32_t tid = 0; tid < RS_NT; tid++) PTBand<E>::vacc(t, tab, band, ib, chunk, group, tid, lds, *reinterpret_cast<Sum *>(&acc[16 * tid]));
            }
            for (uint32_t tid = 0; tid < RS_NT; tid++) PTBand<E>::vput(t, band, group, tid, *reinterpret_cast<Sum *>(&acc[16 * tid]), lds);
        }
    }
}

// resample_run_kernel / resample_tensor_run_kernel (csrc/resample.hip, resample_run_body): the workgroups of the runs of `bpr` bands, phase by
// phase.  The move of the kept rows overlaps itself, and this emulation runs a phase's lanes one after another — which would hide exactly
// that hazard if a lane read and wrote in one go.  So a slab's READ phase runs for all lanes (each lane's registers kept apart), then its
// WRITE phase.  phases == 0 runs the move the wrong way on purpose, every lane reading and writing in turn: the test shows that this
// emulation catches it.  moved: dwords moved; reused: source rows that skipped the horizontal pass.
template <class V>
void run_runs(const ResampleJob &j, const int32_t *tab, uint32_t bpr, uint32_t phases, uint8_t *lds, uint32_t lds_total, uint64_t &moved, uint64_t &reused,
              const V &vstore) {
    std::vector<uint32_t> regs(RS_NT * RS_ROLL_DW);
    typedef uint32_t Reg[RS_ROLL_DW];
    for (uint32_t band0 = 0; band0 < j.bands; band0 += bpr) {
        const uint32_t band1 = band0 + bpr < j.bands ? band0 + bpr : j.bands;
        memset(lds, 0xCD, lds_total);  // garbage, like real LDS, once per workgroup
        vstore.begin();
        for (uint32_t band = band0; band < band1; band++) {
            if (band == band0) {
                uint32_t r0, r1, s0, s1;
                RBand::rows_of(j, tab, band, r0, r1, s0, s1);
                for (uint32_t t = 0; t < RS_NT; t++) hpass_rows_kind(j, tab, s0, s1 - s0, 0u, t, lds);
            } else {
                uint32_t shift, keep, n0, s0, s1;
                RBand::roll_of(j, tab, band, shift, keep, n0, s0, s1);
                reused += keep;
                if (shift != 0u && keep != 0u) {
                    const uint32_t slabs = RBand::roll_slabs(j, keep);
                    for (uint32_t slab = 0; slab < slabs; slab++) {
                        if (phases) {
                            for (uint32_t t = 0; t < RS_NT; t++) RBand::roll_read(j, shift, keep, slab, t, lds, *reinterpret_cast<Reg *>(&regs[RS_ROLL_DW * t]));
                            for (uint32_t t = 0; t < RS_NT; t++) RBand::roll_write(j, keep, slab, t, lds, *reinterpret_cast<Reg *>(&regs[RS_ROLL_DW * t]));
                        } else {
                            for (uint32_t t = 0; t < RS_NT; t++) {
                                RBand::roll_read(j, shift, keep, slab, t, lds, *reinterpret_cast<Reg *>(&regs[RS_ROLL_DW * t]));
                                RBand::roll_write(j, keep, slab, t, lds, *reinterpret_cast<Reg *>(&regs[RS_ROLL_DW * t]));
                            }
                        }
                    }
                    moved += (uint64_t)keep * (j.pitch >> 2);
                }
                if (keep < s1 - s0) memset(lds + (size_t)keep * j.pitch, 0xCD, (size_t)(s1 - s0 - keep) * j.pitch);  // (what is not kept is garbage again)
                if (s1 > n0)
                    for (uint32_t t = 0; t < RS_NT; t++) hpass_rows_kind(j, tab, n0, s1 - n0, n0 - s0, t, lds);
            }
            for (uint32_t t = 0; t < RS_NT; t++) vstore(band, t);
        }
    }
}

// info of a run emulation: rb, bands, cap_rows, bpr, lds_bytes, runs, bands of the last run, dwords moved, rows reused, source rows read
void run_info(uint32_t *info, const ResampleJob &j, const int32_t *tab, uint32_t bpr, uint64_t moved, uint64_t reused) {
    uint64_t passed = 0;
    uint32_t read = 0;
    resample_band_rows(j, tab, passed, read);
    info[0] = j.rb, info[1] = j.bands, info[2] = j.cap_rows, info[3] = bpr, info[4] = j.lds_bytes, info[5] = (j.bands + bpr - 1u) / bpr;
    info[6] = j.bands - (info[5] - 1u) * bpr, info[7] = (uint32_t)moved, info[8] = (uint32_t)reused, info[9] = read, info[10] = (uint32_t)passed;
}

// the vertical pass of a run's band: what `vstore(band)` is in resample_run_body
struct U8Store {
    const ResampleJob &j;
    const int32_t *tab;
    uint8_t *lds;
    void begin() const {}
    void operator()(uint32_t band, uint32_t t) const { RBand::vstore(j, tab, band, t, lds); }
};
template <class E>
struct TensorStore {
    const TensorJob &t;
    const int32_t *tab;
    const uint32_t *ttab;
    uint8_t *lds;
    void begin() const {
        for (uint32_t tid = 0; tid < RS_NT; tid++) TBand<E>::load_table(t, ttab, tid, lds);
    }
    void operator()(uint32_t band, uint32_t tid) const { TBand<E>::vstore(t, tab, band, tid, lds); }
};

}  // namespace

extern "C" {
// geom = the Geometry above as 14 words.  `src` (any alignment): in_h rows of in_w * nc bytes; `dst` (4-byte aligned): ch rows of
// cw * channels bytes.  Returns 0, -1 when the planner refuses, -3 when the placement shows no pixel.
int emu_filter_u8(const uint32_t *geom, const uint8_t *src, const uint8_t *fill, uint8_t *dst, uint32_t *info) {
    Geometry g;
    memcpy(&g, geom, sizeof g);
    PlacedJob pj{};
    ResampleJob &j = pj.r;
    std::vector<int32_t> tab;
    int rc = plan(g, j, pj.p, tab, fill);
    if (rc) return rc;
    j.src = src, j.dst = dst;
    std::vector<uint8_t> lds_store(j.lds_bytes + 16);
    uint8_t *lds = lds_store.data() + ((16 - ((uintptr_t)lds_store.data() & 15)) & 15);
    uint32_t most = 0;
    if (g.placed) run_placed_u8(pj, tab.data(), lds, most);
    else run_u8(j, tab.data(), lds, most);
    fill_info(info, j, tab, g.placed ? pj.p.bands : j.bands, most);
    return 0;
}
// the tensor kernels: `dst` (16-byte aligned) channel planes of ch * cw elements.  dtype 1 / 2 / 3 = f32 / f16 / bf16.  -2: a refused format.
int emu_filter_tensor(const uint32_t *geom, const uint8_t *src, const uint8_t *fill, uint8_t *dst, uint32_t flip, uint32_t dtype, const float *mean,
                      const float *std_, uint32_t *info) {
    Geometry g;
    memcpy(&g, geom, sizeof g);
    const char *why = nullptr;
    const uint32_t onc = g.kind ? 3u : g.nc;
    if (!tensor_format_ok(dtype, 0, mean, std_, onc, why)) return -2;
    PlacedTensorJob t{};
    ResampleJob &j = t.t.r;
    std::vector<int32_t> tab;
    int rc = plan(g, j, t.p, tab, fill);
    if (rc) return rc;
    j.src = src, j.dst = dst;
    t.t.plane = g.cw * g.ch;
    t.t.flip = flip;
    std::vector<uint32_t> ttab(4 * 256, 0xDEADBEEFu);
    tensor_table(dtype, mean, std_, onc, ttab.data());
    const uint32_t lds_total = ((j.lds_bytes + 15u) & ~15u) + TN_TABLE_MAX;
    std::vector<uint8_t> lds_store(lds_total + 16);
    uint8_t *lds = lds_store.data() + ((16 - ((uintptr_t)lds_store.data() & 15)) & 15);
    uint32_t most = 0;
    const bool wide = tensor_elem_bytes(dtype) == 4u;
    if (g.placed && wide) run_placed_tensor<uint32_t>(t, tab.data(), ttab.data(), lds, lds_total, most);
    else if (g.placed) run_placed_tensor<uint16_t>(t, tab.data(), ttab.data(), lds, lds_total, most);
    else if (wide) run_tensor<uint32_t>(t.t, tab.data(), ttab.data(), lds, lds_total, most);
    else run_tensor<uint16_t>(t.t, tab.data(), ttab.data(), lds, lds_total, most);
    fill_info(info, j, tab, g.placed ? t.p.bands : j.bands, most);
    return 0;
}
// The run kernels.  bpr == 0: what the planner's rule gives (-4 when it keeps the bands); else that many bands per run (-4 when the job
// is no candidate).  phases: see run_runs.
int emu_filter_run_u8(const uint32_t *geom, uint32_t bpr, uint32_t phases, const uint8_t *src, uint8_t *dst, uint32_t *info) {
    Geometry g;
    memcpy(&g, geom, sizeof g);
    if (g.placed) return -1;
    ResampleJob j{};
    Place p{};
    std::vector<int32_t> tab;
    const uint8_t nofill[4] = {0, 0, 0, 0};
    int rc = plan(g, j, p, tab, nofill);
    if (rc) return rc;
    bpr = resample_roll_bpr(j, tab.data(), g.filter, bpr);
    if (!bpr) return -4;
    j.src = src, j.dst = dst;
    std::vector<uint8_t> lds_store(j.lds_bytes + 16);
    uint8_t *lds = lds_store.data() + ((16 - ((uintptr_t)lds_store.data() & 15)) & 15);
    uint64_t moved = 0, reused = 0;
    run_runs(j, tab.data(), bpr, phases, lds, j.lds_bytes, moved, reused, U8Store{j, tab.data(), lds});
    run_info(info, j, tab.data(), bpr, moved, reused);
    return 0;
}
int emu_filter_run_tensor(const uint32_t *geom, uint32_t bpr, uint32_t phases, const uint8_t *src, uint8_t *dst, uint32_t flip, uint32_t dtype, const float *mean,
                          const float *std_, uint32_t *info) {
    Geometry g;
    memcpy(&g, geom, sizeof g);
    if (g.placed) return -1;
    const char *why = nullptr;
    const uint32_t onc = g.kind ? 3u : g.nc;
    if (!tensor_format_ok(dtype, 0, mean, std_, onc, why)) return -2;
    TensorJob t{};
    ResampleJob &j = t.r;
    Place p{};
    std::vector<int32_t> tab;
    const uint8_t nofill[4] = {0, 0, 0, 0};
    int rc = plan(g, j, p, tab, nofill);
    if (rc) return rc;
    bpr = resample_roll_bpr(j, tab.data(), g.filter, bpr);
    if (!bpr) return -4;
    j.src = src, j.dst = dst;
    t.plane = g.cw * g.ch;
    t.flip = flip;
    std::vector<uint32_t> ttab(4 * 256, 0xDEADBEEFu);
    tensor_table(dtype, mean, std_, onc, ttab.data());
    const uint32_t lds_total = ((j.lds_bytes + 15u) & ~15u) + TN_TABLE_MAX;
    std::vector<uint8_t> lds_store(lds_total + 16);
    uint8_t *lds = lds_store.data() + ((16 - ((uintptr_t)lds_store.data() & 15)) & 15);
    uint64_t moved = 0, reused = 0;
    if (tensor_elem_bytes(dtype) == 4u) run_runs(j, tab.data(), bpr, phases, lds, lds_total, moved, reused, TensorStore<uint32_t>{t, tab.data(), ttab.data(), lds});
    else run_runs(j, tab.data(), bpr, phases, lds, lds_total, moved, reused, TensorStore<uint16_t>{t, tab.data(), ttab.data(), lds});
    run_info(info, j, tab.data(), bpr, moved, reused);
    return 0;
}
// the inline table functions that were there before the filters, beside filter 0 of the new ones
uint32_t emu_filter_ksize(uint32_t filter, uint32_t in_size, uint32_t out_size) { return resample_ksize_filtered(filter, in_size, out_size); }
uint32_t emu_filter_ksize_old(uint32_t in_size, uint32_t out_size) { return resample_ksize(in_size, out_size); }
void emu_filter_tables(uint32_t filter, uint32_t in_size, uint32_t out_size, uint32_t first, uint32_t count, int32_t *bounds, int32_t *coefs, uint32_t ksize) {
    resample_coefficients_range_filtered(filter, in_size, out_size, first, count, bounds, coefs, ksize);
}
void emu_filter_tables_old(uint32_t in_size, uint32_t out_size, uint32_t first, uint32_t count, int32_t *bounds, int32_t *coefs, uint32_t ksize) {
    if (first == 0u && count == out_size) resample_coefficients(in_size, out_size, bounds, coefs, ksize);
    else resample_coefficients_range(in_size, out_size, first, count, bounds, coefs, ksize);
}
}
