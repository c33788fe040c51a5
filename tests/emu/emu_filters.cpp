// emu_filters.cpp — TEST-ONLY CPU emulation of the band kernels (csrc/resample.hip, csrc/placed.hip) under the filters of DESIGN.md
// §4.15: the product's filtered tables, its planners and every workgroup of the launch grid through the product's own walks (band_walk / run_walk of
// csrc/band_walk.hpp under the lanes of band_lanes.hpp: the walks' barriers are the phase boundaries).  The kernels do not know the
// filter: they get wider tables with negative weights.  And the run kernels: the workgroups of the runs of bands.
// Built by tests/test_filters_emulation.py (g++, the flags of tests/emu/Makefile).
#include "hip_shim.hpp"
#include "band_lanes.hpp"

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

// info: rb, the job's bands, cap_rows, most chunks of a band, lds_bytes, launch bands, hks, vks, whether a weight of the horizontal /
// the vertical table is negative
void fill_info(uint32_t *info, const ResampleJob &j, const std::vector<int32_t> &tab, uint32_t bands, uint32_t most) {
    if (!info) return;
    info[0] = j.rb, info[1] = j.bands, info[2] = j.cap_rows, info[3] = most, info[4] = j.lds_bytes, info[5] = bands, info[6] = j.hks, info[7] = j.vks;
    info[8] = info[9] = 0;
    for (size_t i = j.hk; i < j.vb; i++) info[8] |= tab[i] < 0;
    for (size_t i = j.vk; i < tab.size(); i++) info[9] |= tab[i] < 0;
}

// resample_run_kernel / resample_tensor_run_kernel (csrc/resample.hip): the workgroups of the runs of `bpr` bands through the product's
// run_walk.  `begin(lanes)`: the kernel's prologue; `vstore(band, tid)`: its vertical pass.  moved (dwords moved) and reused (source rows
// that skipped the horizontal pass) are counted beside the walk, from RBand::roll_of.
template <class L, class P, class V>
void run_runs(const ResampleJob &j, const int32_t *tab, uint32_t bpr, HostLds &lds, uint64_t &moved, uint64_t &reused, const P &begin, const V &vstore) {
    for (uint32_t band = 1; band < j.bands; band++) {
        if (band % bpr == 0u) continue;  // (the first band of a run keeps nothing)
        uint32_t shift, keep, n0, s0, s1;
        RBand::roll_of(j, tab, band, shift, keep, n0, s0, s1);
        reused += keep;
        if (shift != 0u && keep != 0u) moved += (uint64_t)keep * (j.pitch >> 2);
    }
    for (uint32_t band0 = 0; band0 < j.bands; band0 += bpr) {
        const uint32_t band1 = min(band0 + bpr, j.bands);
        lds.fresh();
        L lanes;
        begin(lanes);
        with_kind(j.src_nc, [&](auto k) { run_walk<decltype(k)::value>(j, tab, band0, band1, lds.p, vstore, lanes); });
    }
}

// The negative control (phases == 0): lanes under which the move of the kept rows runs the wrong way, every lane reading and writing
// its slab in one go.  The move overlaps itself, so a lane's write lands on a dword a later lane has yet to read; the test shows that
// this emulation, which runs lanes one after another, sees it.  Everything else of the run is run_walk's.
struct OneGoLanes : HostLanes {};
// (run_walk's call of roll_move finds this one for these lanes)
void roll_move(const ResampleJob &j, uint32_t shift, uint32_t keep, uint8_t *lds, OneGoLanes &lanes) {
    const uint32_t slabs = RBand::roll_slabs(j, keep);
    for (uint32_t slab = 0; slab < slabs; slab++)
        lanes.each([=, &j](uint32_t tid) {
            uint32_t reg[RS_ROLL_DW];
            RBand::roll_read(j, shift, keep, slab, tid, lds, reg);
            RBand::roll_write(j, keep, slab, tid, lds, reg);
        });
    lanes.barrier();
}

// info of a run emulation: rb, bands, cap_rows, bpr, lds_bytes, runs, bands of the last run, dwords moved, rows reused, source rows read
void run_info(uint32_t *info, const ResampleJob &j, const int32_t *tab, uint32_t bpr, uint64_t moved, uint64_t reused) {
    uint64_t passed = 0;
    uint32_t read = 0;
    resample_band_rows(j, tab, passed, read);
    info[0] = j.rb, info[1] = j.bands, info[2] = j.cap_rows, info[3] = bpr, info[4] = j.lds_bytes, info[5] = (j.bands + bpr - 1u) / bpr;
    info[6] = j.bands - (info[5] - 1u) * bpr, info[7] = (uint32_t)moved, info[8] = (uint32_t)reused, info[9] = read, info[10] = (uint32_t)passed;
}

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
    uint32_t most = 0, fill_bands = 0;
    if (g.placed) emu_launch_placed(pj, tab.data(), most, fill_bands);
    else emu_launch_u8(j, tab.data(), most);
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
    uint32_t most = 0, fill_bands = 0;
    const bool wide = tensor_elem_bytes(dtype) == 4u;
    if (g.placed && wide) emu_launch_placed_tensor<uint32_t>(t, tab.data(), ttab.data(), most, fill_bands);
    else if (g.placed) emu_launch_placed_tensor<uint16_t>(t, tab.data(), ttab.data(), most, fill_bands);
    else if (wide) emu_launch_tensor<uint32_t>(t.t, tab.data(), ttab.data(), most);
    else emu_launch_tensor<uint16_t>(t.t, tab.data(), ttab.data(), most);
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
    HostLds lds(j.lds_bytes);
    uint64_t moved = 0, reused = 0;
    auto begin = [](HostLanes &) {};
    auto vstore = [&](uint32_t band, uint32_t tid) { RBand::vstore(j, tab.data(), band, tid, lds.p); };
    if (phases) run_runs<HostLanes>(j, tab.data(), bpr, lds, moved, reused, begin, vstore);
    else run_runs<OneGoLanes>(j, tab.data(), bpr, lds, moved, reused, begin, vstore);
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
    HostLds lds(host_tensor_lds(j));
    uint64_t moved = 0, reused = 0;
    const bool wide = tensor_elem_bytes(dtype) == 4u;
    auto begin = [&](HostLanes &lanes) {
        lanes.each([&](uint32_t tid) { wide ? TBand<uint32_t>::load_table(t, ttab.data(), tid, lds.p) : TBand<uint16_t>::load_table(t, ttab.data(), tid, lds.p); });
    };
    auto vstore = [&](uint32_t band, uint32_t tid) {
        wide ? TBand<uint32_t>::vstore(t, tab.data(), band, tid, lds.p) : TBand<uint16_t>::vstore(t, tab.data(), band, tid, lds.p);
    };
    if (phases) run_runs<HostLanes>(j, tab.data(), bpr, lds, moved, reused, begin, vstore);
    else run_runs<OneGoLanes>(j, tab.data(), bpr, lds, moved, reused, begin, vstore);
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
