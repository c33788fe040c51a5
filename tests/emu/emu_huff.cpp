// emu_huff.cpp — TEST-ONLY CPU run of the device entropy decoder (csrc/huff_sync_core.hpp: sync passes with speculative emission,
// block numbering, expansion) on the plan the host front-end makes (Frontend::plan_device_scans).
#include <algorithm>
#include <cstdlib>
#include <cstdio>
#include "hip_shim.hpp"
#include <vector>
#include "../../jpeg-decoder_amd/csrc/host/frontend.hpp"
#include "../../jpeg-decoder_amd/csrc/huff_core.hpp"
#include "../../jpeg-decoder_amd/csrc/huff_sync_core.hpp"

using namespace jpgpu;
using jpgpu::host::Frontend;
using jpgpu::host::PlannedScan;

static uint32_t g_sync_iters = 1, g_sync_wg = 256, g_sync_stale = 0;  // launch shape of the sync passes (emu_huff_set_launch)
static uint32_t g_late = 2;  // HuffSyncJob::late_pass (emu_huff_set_late)
static uint32_t g_tail = 8;  // eighths of its chunk a lane walks in sync pass 0 (HuffSyncJob::pass0_skip)
static uint32_t g_chunk_blocks = 48, g_chunk_min_shift = 10, g_max_launches = 32;  // chunking and launches (emu_huff_set_chunking; batch_entropy.cpp picks them per call)
static uint32_t g_dri_shift = 0;  // restart segments in chunk slots: forced chunk size (emu_huff_set_dri; 0: the product's choice)
static uint32_t g_emit_mismatch = 0;
static uint32_t g_range[2] = {0, 0};  // by-product of the last emu_huff_decode: largest |DC * q| / |AC * q| written (range_stats.hpp)

// What huff_expand_kernel (csrc/huff.hip) does with the settled emission lists, one entry after the other: a block belongs to
// the chunk it starts in; its entries may run on through the leading entries of the chunks that follow.  Every block below the
// scan's total is written whole (the planes are NOT zero-filled on this path: the caller fills them with a pattern).
static void emu_expand(const HuffSyncJob& sj, HuffRange& rg) {
    for (uint32_t i = 0; i < sj.n_chunks; i++) {
        const uint32_t cw = sj.emit_cnt[i], cnt = std::min(cw & 0xffffu, sj.emit_stride), lead = std::min(cw >> 16, cnt);
        if (lead >= cnt) continue;
        const HuffChunkSpan span = huff_chunk_span(sj, i);
        uint32_t seg_first, seg_blocks;
        huff_segment_blocks(sj, span.seg, seg_first, seg_blocks);
        const uint32_t total = seg_first + seg_blocks;  // blocks (and lists) end with the restart segment, if there are any
        const uint32_t seg_end_chunk = sj.n_seg > 1u ? (span.seg + 1u) * sj.seg_chunks : sj.n_chunks;
        const uint32_t k_i = span.first ? 0u : sj.out_qk[i - 1] & 0xffu;
        uint32_t blk = sj.n_blocks[i] + (k_i ? 1u : 0u);  // the first block that starts here
        const uint32_t w0 = sj.uniform ? 0u : sj.dc_sum[2 * i], w1 = sj.uniform ? 0u : sj.dc_sum[2 * i + 1];
        const uint32_t pred[4] = {w0 & 0xffffu, w0 >> 16, w1 & 0xffffu, w1 >> 16};
        int16_t cur[64];
        bool open = false;
        auto flush = [&]() {
            if (open && blk < total) {
                const uint32_t m = blk / sj.bpm, q = blk - m * sj.bpm, my = m / sj.cols, mx = m - my * sj.cols;
                const HuffScanComp& sc = sj.comp[sj.q_comp[q]];
                const uint32_t sub = sj.q_sub[q], vp = sub / sc.h, hp = sub - vp * sc.h;
                memcpy(sc.dst + ((size_t)(my * sc.v + vp) * sc.block_w + (mx * sc.h + hp)) * 64u, cur, 128);
            }
            if (open) blk++;
            open = false;
        };
        auto put = [&](uint32_t ent) {
            static const uint8_t kUnzig[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                               35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
            const uint32_t c = sj.q_comp[blk % sj.bpm], z = kUnzig[(ent >> 16) & 63u];  // (an entry carries the zig-zag index)
            if (!sj.uniform && c != ((ent >> 22) & 3u)) g_emit_mismatch++;  // (the component the lane wrote into the entry)
            uint32_t v = ent & 0xffffu;
            if (huff_entry_is_dc(ent) && !sj.uniform) v = (v + pred[c]) & 0xffffu;
            cur[z] = (int16_t)(uint16_t)v;
            const int32_t sv = (int16_t)(uint16_t)v;
            const uint32_t a = (uint32_t)(sv < 0 ? -sv : sv) * sj.q[c][z];
            if (blk < total) {
                if (huff_entry_is_dc(ent)) {
                    if (!sj.uniform) rg.dc = std::max(rg.dc, a);
                } else {
                    rg.ac = std::max(rg.ac, a);
                }
            }
        };
        const uint32_t* buf = sj.emit + (size_t)i * sj.emit_stride;
        for (uint32_t e = lead; e < cnt; e++) {
            if (huff_entry_is_dc(buf[e])) {
                flush();
                memset(cur, 0, sizeof(cur));
                open = true;
            }
            put(buf[e]);
        }
        for (uint32_t j = i + 1; open && j < seg_end_chunk; j++) {  // the rest of the last block
            const uint32_t cj = sj.emit_cnt[j], cntj = std::min(cj & 0xffffu, sj.emit_stride), leadj = std::min(cj >> 16, cntj);
            const uint32_t* bj = sj.emit + (size_t)j * sj.emit_stride;
            for (uint32_t e = 0; e < leadj; e++) put(bj[e]);
            if (leadj < cntj) break;
        }
        flush();
    }
}

extern "C" {
// huff_stage_segment / huff_sync_chunk_shift as the product uses them (host-side helpers of csrc/huff_job.hpp)
uint32_t emu_stage_segment(uint8_t* dst, const uint8_t* src, uint32_t n) { return huff_stage_segment(dst, src, n); }
uint32_t emu_slot_bytes(uint32_t n) { return huff_slot_bytes(n); }
int emu_stage_segment_clean(uint8_t* dst, const uint8_t* src, uint32_t n) {
    bool clean = true;
    huff_stage_segment(dst, src, n, &clean);
    return clean ? 1 : 0;
}
uint32_t emu_chunk_shift(uint32_t stuffed_bytes, uint32_t total_blocks) { return huff_sync_chunk_shift(stuffed_bytes, total_blocks); }

void emu_huff_set_dri(uint32_t shift) { g_dri_shift = shift; }
// blocks per chunk aimed at, smallest chunk (1 << min_shift bits), launches a scan is given: 48 / 10 / 32 by default; a small call of the
// product gets 12 / 9 / 16 (two passes each)
void emu_huff_set_chunking(uint32_t blocks, uint32_t min_shift, uint32_t launches) {
    g_chunk_blocks = blocks ? blocks : 48u;
    g_chunk_min_shift = min_shift ? min_shift : 10u;
    g_max_launches = launches ? launches : 32u;
}
void emu_huff_set_late(uint32_t pass) { g_late = pass; }
void emu_huff_set_tail(uint32_t eighths) { g_tail = eighths >= 1 && eighths <= 8 ? eighths : 8; }
void emu_huff_last_range(uint32_t out[2]) { out[0] = g_range[0], out[1] = g_range[1]; }
void emu_huff_set_launch(uint32_t iters, uint32_t workgroup, uint32_t stale) {
    g_sync_stale = stale;
    g_sync_iters = iters ? iters : 1u;
    g_sync_wg = workgroup ? workgroup : 256u;
}
// Returns: -1 not eligible; otherwise the status word (0 = every segment decoded cleanly).  coefs[c] must hold
// block_w*block_h*64 zeros for frame component c (sizes from *desc, filled when eligible).
int emu_huff_plan(const uint8_t* data, size_t len, jpgpu_image_desc* desc, uint32_t* n_scans, uint32_t* n_segments) {
    Frontend fe(data, len);
    std::vector<PlannedScan> scans;
    try {
        fe.read_info();
    } catch (...) {
        return -1;
    }
    if (!fe.plan_device_scans(scans)) return -1;
    memset(desc, 0, sizeof(*desc));
    desc->ncomp = fe.ncomp();
    for (uint32_t c = 0; c < desc->ncomp; c++) {
        desc->components[c] = fe.components()[c];
        memcpy(desc->quantization_tables[c], fe.qtable_of_component(c), 128);
    }
    desc->out_w = fe.output_width();
    desc->out_h = fe.output_height();
    desc->color_transform = fe.color_transform();
    *n_scans = (uint32_t)scans.size();
    *n_segments = 0;
    for (auto& s : scans) *n_segments += (uint32_t)(s.seg_off.size() / 2);
    return 0;
}
// 1: every scan writes all blocks of its planes (huff_scan_covers_planes: batch_entropy.cpp skips the zero fill for such images)
int emu_huff_covered(const uint8_t* data, size_t len) {
    Frontend fe(data, len);
    std::vector<PlannedScan> scans;
    fe.read_info();
    if (!fe.plan_device_scans(scans)) return -1;
    for (const PlannedScan& ps : scans) {
        HuffSyncJob sj;
        memset(&sj, 0, sizeof(sj));
        sj.cols = ps.cols, sj.n_mcu = ps.n_mcu, sj.ncomp = ps.ncomp;
        uint32_t bh[4] = {0, 0, 0, 0};
        for (uint32_t c = 0; c < ps.ncomp; c++) {
            sj.comp[c].block_w = ps.comp[c].block_w, sj.comp[c].h = ps.comp[c].h, sj.comp[c].v = ps.comp[c].v;
            bh[c] = fe.components()[ps.comp[c].frame_index].block_height;
        }
        if (!huff_scan_covers_planes(sj, bh)) return 0;
    }
    return 1;
}
// What the 4:2:0 pixel walk makes of the same settled lists when it reads them itself (csrc/fused_entries.hpp S420E::scatter_row +
// huff.hip huff_strip_index_kernel), one entry after the other and for a strip width `tx`: per (MCU row, strip) the chunk in which the
// run's first block starts and the place of its DC entry; then, chunk by chunk, entries -> blocks by counting DC entries from the chunk's
// first-block number — a segment's first chunk continues nothing, numbers are clamped to the segment's end, a chunk writes no block beyond
// its own segment, the strip's own MCUs take all six blocks, the halo MCU either side only its chroma.  True if every block of the
// planes comes out as emu_expand left it.
static bool emu_entry_walk_equals(const HuffSyncJob& sj, uint32_t tx, uint32_t* where) {
    static const uint8_t kUnzig[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                       35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    const uint32_t cols = sj.cols, rows = sj.n_mcu / cols, tiles_x = (cols + tx - 1u) / tx, all = sj.n_mcu * 6u;
    const uint32_t seg_chunks = sj.n_seg > 1u ? sj.seg_chunks : 0u, seg_blocks = sj.ri * 6u;
    auto seg_end = [&](uint32_t c) { return seg_chunks ? std::min((c / seg_chunks + 1u) * seg_blocks, all) : 0xffffffffu; };
    auto first_block = [&](uint32_t c) {
        const bool continues = c && !(seg_chunks && c % seg_chunks == 0u) && (sj.out_qk[c - 1u] & 0xffu);
        return std::min(sj.n_blocks[c] + (continues ? 1u : 0u), seg_end(c));
    };
    std::vector<std::vector<int16_t>> planes(3);
    const uint32_t bw[3] = {sj.comp[0].block_w, sj.comp[1].block_w, sj.comp[2].block_w};
    planes[0].assign((size_t)bw[0] * 2u * rows * 64u, 0);
    planes[1].assign((size_t)bw[1] * rows * 64u, 0);
    planes[2].assign((size_t)bw[2] * rows * 64u, 0);
    for (uint32_t k = 0; k < rows; k++)
        for (uint32_t s = 0; s < tiles_x; s++) {
            const uint32_t x0m = s * tx, te = std::min(tx, cols - x0m), a = x0m ? x0m - 1u : 0u, b = std::min(x0m + te + 1u, cols);
            const uint32_t B0 = 6u * (k * cols + a), nB = 6u * (b - a);
            // the kernel's search, as it runs it: 64 probes per round, the answer among the probes that say "not above B0" — COUNTED
            // (a ballot's population count), which is only right if the numbers are in order
            uint32_t lo = 0, hi = sj.n_chunks;
            while (hi - lo > 1u) {
                const uint32_t step = (hi - lo + 63u) / 64u;
                uint32_t t = 0;
                for (uint32_t lane = 0; lane < 64u; lane++) {
                    const uint32_t c = lo + lane * step;
                    if (c < hi && first_block(c) <= B0) t++;
                }
                const uint32_t nlo = lo + (t - 1u) * step;
                hi = std::min(hi, nlo + step);
                lo = nlo;
            }
            const uint32_t c0 = lo;
            uint32_t e0 = 0xffffffffu;
            {
                const uint32_t cw = sj.emit_cnt[c0], cnt = std::min(cw & 0xffffu, sj.emit_stride);
                uint32_t want = B0 - first_block(c0);
                for (uint32_t e = std::min(cw >> 16, cnt); e < cnt; e++)
                    if (huff_entry_is_dc(sj.emit[(size_t)c0 * sj.emit_stride + e]) && want-- == 0u) {
                        e0 = e;
                        break;
                    }
            }
            if (e0 == 0xffffffffu) {
                *where = 0x10000u | k;
                return false;
            }
            for (uint32_t c = c0; c < sj.n_chunks; c++) {
                const uint32_t cw = sj.emit_cnt[c], cnt = std::min(cw & 0xffffu, sj.emit_stride);
                const uint32_t S = first_block(c);
                if (c != c0 && S >= B0 + nB + 1u) break;
                const uint32_t end = seg_end(c), nBc = end > B0 ? std::min(nB, end - B0) : 0u;
                const uint32_t w0 = sj.dc_sum[2 * c], w1 = sj.dc_sum[2 * c + 1];
                const uint32_t pred[3] = {w0 & 0xffffu, w0 >> 16, w1 & 0xffffu};
                const int64_t dbase = c == c0 ? 0 : (int64_t)S - (int64_t)B0;
                uint32_t started = 0;
                for (uint32_t e = c == c0 ? e0 : 0u; e < cnt; e++) {
                    const uint32_t ent = sj.emit[(size_t)c * sj.emit_stride + e];
                    const bool dc = huff_entry_is_dc(ent);
                    if (dc) started++;
                    const int64_t d = dbase + (int64_t)started - 1;
                    if (d >= 0 && d < (int64_t)nBc) {
                        const uint32_t mx = a + (uint32_t)d / 6u, q = (uint32_t)d % 6u, comp = q < 4u ? 0u : q - 3u;
                        const bool own = mx >= x0m && mx < x0m + te;
                        if (comp != ((ent >> 22) & 3u)) {
                            *where = 0x20000u | k;
                            return false;
                        }
                        uint32_t v = ent & 0xffffu;
                        if (dc) v = (v + pred[comp]) & 0xffffu;
                        if (comp == 0u && own)
                            planes[0][((size_t)(2u * k + (q >> 1)) * bw[0] + 2u * mx + (q & 1u)) * 64u + kUnzig[(ent >> 16) & 63u]] = (int16_t)(uint16_t)v;
                        else if (comp != 0u)
                            planes[comp][((size_t)k * bw[comp] + mx) * 64u + kUnzig[(ent >> 16) & 63u]] = (int16_t)(uint16_t)v;
                    }
                    if (dbase + (int64_t)started >= (int64_t)nB + 1) break;
                }
            }
        }
    for (uint32_t c = 0; c < 3; c++)
        if (memcmp(planes[c].data(), sj.comp[c].dst, planes[c].size() * 2u) != 0) {
            *where = 0x30000u | c;
            return false;
        }
    return true;
}
static uint32_t g_entry_walk_checked = 0;  // scans the twin above has read since the last emu_huff_entry_walk_checked()
extern "C" uint32_t emu_huff_entry_walk_checked() {
    const uint32_t n = g_entry_walk_checked;
    g_entry_walk_checked = 0;
    return n;
}

extern "C" int emu_huff_decode(const uint8_t* data, size_t len, int16_t* const* coefs, uint32_t* n_passes) {
    Frontend fe(data, len);
    std::vector<PlannedScan> scans;
    fe.read_info();
    if (!fe.plan_device_scans(scans)) return -1;
    uint32_t status = 0;
    HuffRange rg;  // what the kernels fold per wave and raise in the image's statistics words
    for (const PlannedScan& ps : scans) {
        // staging as batch_entropy.cpp does it: every segment unstuffed into its own 16-byte aligned, zero padded slot
        size_t total = 0;
        for (size_t sg = 0; sg + 1 < ps.seg_off.size(); sg += 2) total += huff_slot_bytes(ps.seg_off[sg + 1] - ps.seg_off[sg]);
        std::vector<uint8_t> stage_raw(total + 16);
        uint8_t* stage = stage_raw.data() + ((16 - (reinterpret_cast<uintptr_t>(stage_raw.data()) & 15)) & 15);
        std::vector<uint32_t> table(ps.seg_off.size());
        uint32_t o = 0;
        for (size_t sg = 0; sg + 1 < ps.seg_off.size(); sg += 2) {
            const uint32_t first = ps.seg_off[sg], n = ps.seg_off[sg + 1] - first;
            bool clean = true;
            table[sg] = o;
            table[sg + 1] = huff_stage_segment(stage + o, data + ps.data_off + first, n, ps.check_at_staging ? &clean : nullptr);
            o += huff_slot_bytes(n);
            if (!clean) status |= 1u | 16u;  // (batch_entropy.cpp: the staging pass refuses the stream)
        }
        if (status & 1u) continue;
        // restart-marker streams (batch_entropy.cpp, dri_geom): every segment in chunk slots of its own; one segment = a scan without markers
        const bool dri_chunked = ps.ri != 0 && ps.seg_off.size() >= 4;
        {  // the self-synchronising chunk decoder, passes run one after the other
            HuffSyncLds* S = new HuffSyncLds;
            HuffSyncJob& sj = S->job;
            memset(&sj, 0, sizeof(sj));
            uint32_t changed = 0;
            sj.data = stage;
            sj.tables = ps.tables->t;
            sj.status = &status;
            sj.changed = &changed;
            sj.n_bits = table[1] * 8u;
            sj.cols = ps.cols;
            sj.n_mcu = ps.n_mcu;
            sj.ncomp = ps.ncomp;
            for (uint32_t c = 0; c < ps.ncomp; c++) {
                sj.comp[c].dst = coefs[ps.comp[c].frame_index];
                sj.comp[c].block_w = ps.comp[c].block_w;
                sj.comp[c].h = ps.comp[c].h;
                sj.comp[c].v = ps.comp[c].v;
                sj.comp[c].dc = ps.comp[c].dc;
                sj.comp[c].ac = ps.comp[c].ac;
                memcpy(sj.q[c], fe.qtable_of_component(ps.comp[c].frame_index), 128);
            }
            huff_sync_finish_job(sj);
            if (dri_chunked) {
                uint32_t stuffed = 0, longest = 0;
                for (size_t sg = 0; sg + 1 < ps.seg_off.size(); sg += 2) {
                    stuffed += ps.seg_off[sg + 1] - ps.seg_off[sg];
                    longest = std::max<uint32_t>(longest, ps.seg_off[sg + 1] - ps.seg_off[sg]);
                }
                sj.chunk_shift = g_dri_shift ? g_dri_shift : huff_sync_chunk_shift(stuffed, sj.bpm * ps.n_mcu, g_chunk_blocks, g_chunk_min_shift);
                sj.seg_off = table.data();
                sj.n_seg = (uint32_t)(ps.seg_off.size() / 2);
                sj.ri = ps.ri;
                sj.seg_chunks = huff_sync_chunks(longest, sj.chunk_shift);
                sj.n_chunks = sj.n_seg * sj.seg_chunks;
                sj.n_bits = 0;
            } else {
                sj.chunk_shift = huff_sync_chunk_shift(ps.seg_off[1] - ps.seg_off[0], sj.bpm * ps.n_mcu, g_chunk_blocks, g_chunk_min_shift);
                sj.n_chunks = huff_sync_chunks(table[1], sj.chunk_shift);
            }
            sj.pass0_skip = ((1u << sj.chunk_shift) >> 3) * (8u - g_tail);
            sj.late_pass = g_late;
            std::vector<uint32_t> emit_buf, emit_cnt;
            sj.emit_stride = huff_emit_stride(sj.chunk_shift);
            emit_buf.assign((size_t)sj.n_chunks * sj.emit_stride + 1, 0xABABABABu);  // (+1: a canary behind the last buffer)
            emit_cnt.assign(sj.n_chunks, 0xCDCDCDCDu);
            sj.emit = emit_buf.data();
            sj.emit_cnt = emit_cnt.data();
            std::vector<uint32_t> arr(8 * (size_t)sj.n_chunks, 0xCDCDCDCDu);
            sj.blk_end = arr.data() + 7 * (size_t)sj.n_chunks;
            sj.in_pos = arr.data();
            sj.in_qk = arr.data() + sj.n_chunks;
            sj.out_pos = arr.data() + 2 * (size_t)sj.n_chunks;
            sj.out_qk = arr.data() + 3 * (size_t)sj.n_chunks;
            sj.n_blocks = arr.data() + 4 * (size_t)sj.n_chunks;
            sj.dc_sum = arr.data() + 5 * (size_t)sj.n_chunks;
            if (g_sync_stale)  // what a previous batch of similar streams leaves in the arrays: states that LOOK right
                for (uint32_t i = 0; i < sj.n_chunks; i++) {
                    sj.out_pos[i] = ((i + 1u) << sj.chunk_shift) + (i * 7u + g_sync_stale) % 33u;
                    sj.out_qk[i] = (((i * 5u + g_sync_stale) % sj.bpm) << 8) | ((i * 11u) % 64u);
                    sj.in_pos[i] = sj.out_pos[i ? i - 1 : 0];
                    sj.in_qk[i] = sj.out_qk[i ? i - 1 : 0];
                    sj.n_blocks[i] = i % 9u;
                }
            // (huff_weave_kernel) the staged scan, 64 chunks side by side: what the passes read
            sj.data_dwords = (uint32_t)(total / 4);
            std::vector<uint32_t> weave(huff_weave_dwords(sj.n_chunks, sj.chunk_shift) + 1, 0xEFEFEFEFu);
            for (uint32_t i = 0; i < (sj.n_chunks + HUFF_WEAVE_LANES - 1u) / HUFF_WEAVE_LANES * HUFF_WEAVE_LANES; i++)
                for (uint32_t r = 0; r < huff_weave_height(sj.chunk_shift); r++)
                    weave[huff_weave_at(sj.chunk_shift, i, r)] = i < sj.n_chunks ? huff_weave_value(sj, huff_chunk_span(sj, i).start >> 5, r) : 0u;
            sj.weave = weave.data();
            memcpy(S->tables, ps.tables->t, sizeof(S->tables));
            for (uint32_t t = 0; t < 512; t++) huff_sync_fill_lds(*S, t);
            // Launches as huff.hip runs them: workgroups of 256 lanes, `iters` iterations each with a barrier in between.
            // Lanes of a workgroup run concurrently (every lane sees the states its neighbours had before the iteration);
            // workgroups run one after the other here, last first — each sees its left neighbour's state of the previous
            // launch, the least the device guarantees.
            const uint32_t iters = g_sync_iters, WG = g_sync_wg;
            uint32_t pass = 0, launch = 0;
            for (; launch < g_max_launches; launch++) {
                changed = 0;
                const uint32_t n_wg = (sj.n_chunks + WG - 1) / WG;
                for (uint32_t w = n_wg; w-- > 0;) {
                    const uint32_t lo = w * WG, hi = std::min(sj.n_chunks, lo + WG);
                    for (uint32_t it = 0; it < iters; it++) {
                        const uint32_t first = lo ? lo - 1 : 0;
                        std::vector<uint32_t> prev_pos(sj.out_pos + first, sj.out_pos + hi), prev_qk(sj.out_qk + first, sj.out_qk + hi);
                        std::vector<uint32_t> new_pos(prev_pos), new_qk(prev_qk);
                        for (uint32_t i = lo; i < hi; i++) {
                            std::copy(prev_pos.begin(), prev_pos.end(), sj.out_pos + first);
                            std::copy(prev_qk.begin(), prev_qk.end(), sj.out_qk + first);
                            changed += huff_sync_chunk(*S, i, launch * iters + it) ? 1u : 0u;
                            new_pos[i - first] = sj.out_pos[i];
                            new_qk[i - first] = sj.out_qk[i];
                        }
                        std::copy(new_pos.begin(), new_pos.end(), sj.out_pos + first);
                        std::copy(new_qk.begin(), new_qk.end(), sj.out_qk + first);
                    }
                }
                if (getenv("EMU_HUFF_TRACE")) fprintf(stderr, "launch %u changed %u of %u\n", launch, changed, sj.n_chunks);
                if (launch > 0 && changed == 0) break;
            }
            pass = launch;
            if (pass == g_max_launches) status |= 1u | 64u;
            if (sj.n_seg > 1u) {  // (huff_sync_scan_kernel, restart segments: one thread per segment)
                for (uint32_t seg = 0; seg < sj.n_seg; seg++) status |= huff_emit_segment_scan(sj, seg);
                if (emit_buf.back() != 0xABABABABu) status |= 0x8000u;
            } else {
                uint32_t run = 0;
                for (uint32_t i = 0; i < sj.n_chunks; i++) {  // exclusive scan
                    const uint32_t nb = sj.n_blocks[i];
                    sj.n_blocks[i] = run;
                    run += nb;
                    status |= huff_emit_chunk_status(sj, i, run);
                }
                status |= huff_emit_final_status(sj, run);
                if (emit_buf.back() != 0xABABABABu) status |= 0x8000u;  // a lane wrote past its buffer
                if (!sj.uniform) {  // (huff_sync_scan_kernel) sums of DC differences -> predictors at the start of every chunk
                    uint32_t acc[4] = {0, 0, 0, 0};
                    for (uint32_t i = 0; i < sj.n_chunks; i++) {
                        const uint32_t w0 = sj.dc_sum[2 * i], w1 = sj.dc_sum[2 * i + 1];
                        const uint32_t v[4] = {w0 & 0xffffu, w0 >> 16, w1 & 0xffffu, w1 >> 16};
                        sj.dc_sum[2 * i] = (acc[0] & 0xffffu) | ((acc[1] & 0xffffu) << 16);
                        sj.dc_sum[2 * i + 1] = (acc[2] & 0xffffu) | ((acc[3] & 0xffffu) << 16);
                        for (int f = 0; f < 4; f++) acc[f] += v[f];
                    }
                }
            }
            if (status == 0) {
                g_emit_mismatch = 0;
                emu_expand(sj, rg);
                if (g_emit_mismatch) status |= 0x4000u;  // entries that name another component than the block numbering does
                // the entry-list walk's reading of the same lists (batch_entropy.cpp's eligibility rule): strips of 42, 3 and 1 MCUs
                bool walk = ps.ncomp == 3 && !sj.uniform && sj.bpm == 6u && scans.size() == 1 && sj.n_mcu % sj.cols == 0;
                for (uint32_t c = 0; walk && c < 3; c++)
                    walk = ps.comp[c].frame_index == c && ps.comp[c].h == (c ? 1u : 2u) && ps.comp[c].v == (c ? 1u : 2u);
                if (walk && status == 0) {
                    uint32_t bh[4] = {0, 0, 0, 0};
                    for (uint32_t c = 0; c < 3; c++) bh[c] = fe.components()[c].block_height;
                    walk = huff_scan_covers_planes(sj, bh);
                }
                if (walk && status == 0) {
                    uint32_t where = 0;
                    for (uint32_t tx : {42u, 3u, 1u})
                        if (!emu_entry_walk_equals(sj, tx, &where)) {
                            if (getenv("EMU_HUFF_TRACE")) fprintf(stderr, "entry walk twin differs: tx %u where %x\n", tx, where);
                            status |= 0x2000u;
                        }
                    g_entry_walk_checked++;
                }
            }
            // (huff_dc_prefix_kernel, uniform scans only) DC differences -> values, per component in stream order (i16 wrapping)
            for (uint32_t c = 0; sj.uniform && c < ps.ncomp; c++) {
                const HuffScanComp& sc = sj.comp[c];
                const uint32_t hv = sc.h * sc.v;
                uint16_t acc = 0;
                for (uint32_t m = 0; m < sj.n_mcu; m++)
                    for (uint32_t sub = 0; sub < hv; sub++) {
                        if (sj.n_seg > 1u && sub == 0 && m % sj.ri == 0) acc = 0;  // (a restart: the predictor starts again)
                        const uint32_t my = m / sj.cols, mx = m - my * sj.cols, vp = sub / sc.h, hp = sub - vp * sc.h;
                        int16_t* blk = sc.dst + ((size_t)(my * sc.v + vp) * sc.block_w + (mx * sc.h + hp)) * 64u;
                        acc = (uint16_t)(acc + (uint16_t)blk[0]);
                        blk[0] = (int16_t)acc;
                        const int32_t v = (int16_t)acc;  // (the kernel ranges the finished DC values of such a scan)
                        rg.dc = std::max(rg.dc, (uint32_t)(v < 0 ? -v : v) * sj.q[c][0]);
                    }
            }
            if (n_passes) *n_passes = pass;
            delete S;
        }
    }
    g_range[0] = rg.dc, g_range[1] = rg.ac;
    return (int)status;
}
}

