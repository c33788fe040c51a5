// batch_entropy.cpp — the device entropy and progressive launches of a batch (huff.hip, huff_prog_wave.hpp): staging of the scans'
// bytes, tables and job records, the launches, and what the pipeline reads back of them.  Shares struct jpgpu_batch with batch.cpp
// (batch_internal.hpp) and nothing else.
#include <atomic>
#include <chrono>
#include <functional>

#include "batch_internal.hpp"
#include "host/frontend.hpp"

// staged bytes of the device-entropy route: pinned block -> its device twin (offsets and lengths are multiples of 16 by construction)
static hipError_t upload_staged(void *d_dst, const void *h_src, size_t bytes, hipStream_t s) {
    static const bool by_kernel = getenv("JPGPU_UPLOAD_BY_KERNEL") != nullptr;
    void *mapped = nullptr;
    if (by_kernel && ((uintptr_t)h_src & 15u) == 0 && ((uintptr_t)d_dst & 15u) == 0 && hipHostGetDevicePointer(&mapped, const_cast<void *>(h_src), 0) == hipSuccess)
        return launch_copy_from_host(d_dst, mapped, bytes, s);
    if (by_kernel) (void)hipGetLastError();
    return hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, s);
}

// ---- device entropy decoding -----------------------------------------------------------------------------------
// Staging block layout (same offsets in the pinned and the device copy):
//   [ status: n x u32 | settle counters: 4 x u32 per sync job | HuffSyncJob[] (segment jobs) | HuffSyncJob[] (chunk jobs) |
//     DevHuffTable[8] per scan | segment offsets | scan bytes ]   + device only: per-chunk state of the sync jobs
// The range statistics of the decoded coefficients are a by-product of the kernels that write them (HuffSyncJob::stats ->
// the batch's d_stats; round 2 ran range_scan_kernel over the arena afterwards and read the result back).
namespace {
// A scan as the file holds it, into the pinned staging block (host light): the destination is read by the copy engine and never by
// this CPU, so the stores go past the caches — a plain memcpy of 400 kB reads every destination line before it overwrites it, and
// the staging team of a sub-batch is bound by exactly that traffic (25 MB per 64 files: 0.7-0.8 ms on 16 CPUs, the launches of a
// 256-file call one after the other).  JPGPU_STAGE_PLAIN_MEMCPY=1: memcpy (A/B).
inline void copy_past_the_caches(uint8_t *dst, const uint8_t *src, size_t n) {
#if defined(__x86_64__) && defined(__clang__)
    static const bool plain = getenv("JPGPU_STAGE_PLAIN_MEMCPY") != nullptr;
    if (plain || n < 4096u) {
        memcpy(dst, src, n);
        return;
    }
    typedef long long v2di __attribute__((vector_size(16)));
    const size_t head = (16u - ((uintptr_t)dst & 15u)) & 15u;
    memcpy(dst, src, head);
    dst += head, src += head, n -= head;
    size_t i = 0;
    for (; i + 64u <= n; i += 64u) {
        v2di a, b, c, d;
        memcpy(&a, src + i, 16), memcpy(&b, src + i + 16, 16), memcpy(&c, src + i + 32, 16), memcpy(&d, src + i + 48, 16);
        __builtin_nontemporal_store(a, (v2di *)(dst + i));
        __builtin_nontemporal_store(b, (v2di *)(dst + i + 16));
        __builtin_nontemporal_store(c, (v2di *)(dst + i + 32));
        __builtin_nontemporal_store(d, (v2di *)(dst + i + 48));
    }
    __builtin_ia32_sfence();
    memcpy(dst + i, src + i, n - i);
#else
    memcpy(dst, src, n);
#endif
}
struct LaunchClock {  // JPGPU_PIPE_TRACE: where a slow launch spent its time (host)
    bool on = getenv("JPGPU_PIPE_TRACE") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), last = t0;
    char text[512];
    size_t used = 0;
    void mark(const char *what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        used += (size_t)snprintf(text + used, used < sizeof(text) ? sizeof(text) - used : 0, " %s %.2f", what, std::chrono::duration<double, std::milli>(now - last).count());
        if (used >= sizeof(text)) used = sizeof(text) - 1;
        last = now;
    }
    ~LaunchClock() {
        if (on && std::chrono::duration<double, std::milli>(last - t0).count() > 3.0) fprintf(stderr, "pipeline trace: slow device entropy launch (ms):%s\n", text);
    }
};
}  // namespace

int jpgpu::batch_device_entropy_launch(jpgpu_batch *b, const DeviceEntropyImage *images, uint32_t n, void *hip_stream,
                                       const std::function<void(uint32_t, const std::function<void(uint32_t)> &)> *par, void *copy_stream,
                                       DeviceScratch *scratch, bool alone, uint32_t mode, uint32_t *n_light, uint32_t *n_entry) {
    if (!b || !images || n == 0) return JPGPU_ERR_FORMAT;
    LaunchClock clk;
    int rc = use_device(b->device, b->err);
    if (rc) return rc;
    if (!b->d_coef) return set_err(b->err, JPGPU_ERR_FORMAT, "batch has no device buffers bound");
    hipStream_t s = (hipStream_t)hip_stream;
    // Chunk size of the chunk decoder: ~48 blocks per chunk settle in the fewest passes and give the best throughput when a
    // call fills the device (256 x 1080p: 270 k lanes).  A call with few streams is latency-bound instead — three passes in
    // which every lane walks its whole chunk, ~2.4 us per symbol: one 1080p image is 1,055 lanes and 2.3 ms — so small calls
    // get smaller chunks and more (cheap once settled) passes: 1080p 3.07 -> 1.68 ms, 2160p 4.82 -> 3.02, 512^2 2.25 -> 1.30
    // through jpgpu_pipeline_decode (profiles/round2/09_decoder_latency.txt).  The environment knobs pin the values (A/B).
    static const bool sync_pinned = getenv("JPGPU_SYNC_BLOCKS") || getenv("JPGPU_SYNC_MIN_SHIFT") || getenv("JPGPU_SYNC_LAUNCHES");
    static const uint32_t env_sync_blocks = env_u32("JPGPU_SYNC_BLOCKS", 48, 1, 1024);      // blocks per chunk aimed at
    static const uint32_t env_sync_min_shift = env_u32("JPGPU_SYNC_MIN_SHIFT", 10, 7, 15);  // smallest chunk: 1 << this many bits
    static const uint32_t env_sync_launches = env_u32("JPGPU_SYNC_LAUNCHES", 10, 1, 64);
    uint32_t sync_blocks = env_sync_blocks, sync_min_shift = env_sync_min_shift, sync_launches = env_sync_launches;
    // Passes per launch: a call that fills the device runs one pass per launch — launches cost 5 us once a job has settled, and passes
    // that begin with everything the one before published need fewer of them (4,096 files: 53 ms against 55-57 with two passes per
    // launch) —; small calls, which wait for every launch, keep two.
    static const bool iters_pinned = getenv("JPGPU_SYNC_ITERS") != nullptr;
    static const uint32_t env_iters = env_u32("JPGPU_SYNC_ITERS", 2, 1, 8);
    uint32_t sync_iters = env_iters;
    static const uint32_t env_late = env_u32("JPGPU_SYNC_LATE_PASS", 0, 0, 64);  // (0: chosen here)
    uint32_t late_pass = env_late ? env_late : HUFF_LATE_PASS;
    if (!sync_pinned) {
        uint64_t lanes = 0;  // at the throughput setting
        for (uint32_t k = 0; k < n && images[k].scans; k++)
            for (const host::PlannedScan &ps : *images[k].scans)
                if (ps.seg_off.size() >= 2) {  // (restart segments go through the chunk decoder too: about as many lanes for the same bytes)
                    uint32_t blocks = 0;
                    for (uint32_t c = 0; c < ps.ncomp; c++) blocks += ps.comp[c].h * ps.comp[c].v;
                    uint64_t bytes = 0;
                    for (size_t sg = 0; sg + 1 < ps.seg_off.size(); sg += 2) bytes += ps.seg_off[sg + 1] - ps.seg_off[sg];
                    if (bytes < (1u << 28)) lanes += huff_sync_chunks((uint32_t)bytes, huff_sync_chunk_shift((uint32_t)bytes, blocks * ps.n_mcu, 48u, 10u));
                }
        if (lanes < 16384u) sync_blocks = 12u, sync_min_shift = 9u, sync_launches = 16u;
        else if (lanes < 65536u) sync_blocks = 24u, sync_launches = 12u;
        else {
            if (!iters_pinned) sync_iters = 1u, sync_launches = 16u;
            // one of many sub-batches in flight: what counts is the work, and longer chunks mean fewer lanes that decode their chunk twice
            // (4,096 files: 50.4-55.2 ms against 51.3-60.0 on one box, interleaved; a call of one or two sub-batches waits for the chains
            // of its late passes instead and keeps the shorter ones: tools/gpu_knobs3.sh)
            if (!alone) sync_blocks = 64u;
        }
    }
    // Speculative emission (huff_job.hpp): the sync passes leave entry lists, huff_expand_kernel writes whole blocks — no write
    // pass, and no zero fill for images whose scans cover their planes.
    bool low_table_ids = env_u32("JPGPU_SYNC_COMPACT_TABLES", 1, 0, 1) != 0;  // until a scan uses a Huffman table id above 1 (huff_sync_pass_kernel<4>)
    static const bool tail_pinned = getenv("JPGPU_SYNC_TAIL") != nullptr;
    static const uint32_t env_tail = env_u32("JPGPU_SYNC_TAIL", 3, 1, 8);  // eighths of its chunk a lane walks in the first sync pass
    const uint32_t sync_tail = (alone && !tail_pinned) ? 8u : env_tail;
    if (alone && !iters_pinned) sync_iters = env_iters;
    // Restart-marker streams (huff_job.hpp, HuffSyncJob::seg_chunks): every segment gets chunk slots of its own (`uniform` scans
    // too: huff_dc_prefix_kernel starts its sums again at every segment); a scan whose restart interval covers all its MCUs is ONE
    // segment, i.e. a scan without restart markers.  Bit positions are 32-bit numbers relative to the scan's first slot: a scan
    // whose slots exceed 2^29 bytes is handed back to the host (status bit 8).
    struct DriGeom {
        bool chunked, too_large;
        uint32_t shift, seg_chunks;
    };
    auto dri_geom = [&](const host::PlannedScan &ps) {
        DriGeom g{false, false, 0u, 0u};
        if (ps.ri == 0 || ps.seg_off.size() < 4) return g;
        uint32_t blocks = 0;
        for (uint32_t c = 0; c < ps.ncomp; c++) blocks += ps.comp[c].h * ps.comp[c].v;
        uint64_t stuffed = 0, slots = 0;
        uint32_t longest = 0;
        for (size_t sg = 0; sg + 1 < ps.seg_off.size(); sg += 2) {
            stuffed += ps.seg_off[sg + 1] - ps.seg_off[sg];
            slots += huff_slot_bytes(ps.seg_off[sg + 1] - ps.seg_off[sg]);
            longest = std::max<uint32_t>(longest, ps.seg_off[sg + 1] - ps.seg_off[sg]);
        }
        g.chunked = true;
        if (stuffed >= (1u << 28) || slots >= (1u << 29)) {
            g.too_large = true;
            return g;
        }
        g.shift = huff_sync_chunk_shift((uint32_t)stuffed, blocks * ps.n_mcu, sync_blocks, sync_min_shift);
        g.seg_chunks = huff_sync_chunks(longest, g.shift);
        return g;
    };
    rc = batch_enable_dev_classes(b);
    if (rc) return rc;
    // "Host light" (include/jpgpu_decoder.h): scans without restart markers go up as the file holds them — the staging task is a plain
    // memcpy, or nothing at all when the caller's buffers are pinned (DEVICE_ENTROPY_INPUT_PINNED: the copy engine reads them) — into a
    // MIRROR of the data area, and huff_unstuff_* (huff.hip) does what huff_stage_segment does: marker check, unstuffing into the
    // scan's slot, the job record's lengths.  Scans with restart markers are staged by the host as ever (into the mirror too: their
    // jobs then read them there).
    const bool light = (mode & DEVICE_ENTROPY_LIGHT) != 0, input_pinned = light && (mode & DEVICE_ENTROPY_INPUT_PINNED) != 0;
    // Entry-list pixel path: which 4:2:0 strip walk (if any) a batch image belongs to
    const bool entry_pixels = (mode & DEVICE_ENTROPY_ENTRY_PIXELS) != 0;
    std::vector<const FusedGeom *> walk_geom(entry_pixels ? b->descs.size() : 0, nullptr);
    if (entry_pixels)
        for (const FusedPlan &fp : b->fused)
            if (fp.kind == FUSED_420 && fp.strip)
                for (uint32_t i = 0; i < fp.n_images; i++) walk_geom[fp.ids[i]] = &fp.geoms[i];
    batch_drop_entries(b);
    // Windowed images: which rows of their scan the window kernel reads (the others need not reach the arena)
    std::vector<const WindowGeom *> win_geom((mode & DEVICE_ENTROPY_WINDOW_ROWS) && !b->win.ids.empty() ? b->descs.size() : 0, nullptr);
    for (size_t k = 0; k < b->win.ids.size() && !win_geom.empty(); k++) win_geom[b->win.ids[k]] = &b->win.geoms[k];
    size_t n_raw_jobs = 0;
    uint32_t max_pieces = 0, light_images = 0;
    constexpr size_t PINNED_SPAN_GAP_MAX = 4096u;  // (bytes; below one page: see where the spans are built)
    struct PinnedSpan {
        const uint8_t *start, *end;  // the caller's bytes [start, end): the scans of consecutive files and what lies between them
        size_t mirror_off;           // where `start` lands in the span region of the mirror
    };
    std::vector<PinnedSpan> spans;
    std::vector<size_t> raw_mirror_off;  // per raw scan, in listing order: its offset in the span region
    struct RawScan {
        const uint8_t *src;
        size_t bytes, listed;  // (listed: its place in listing order)
    };
    std::vector<RawScan> raw_scans;
    size_t n_sync_jobs = 0, seg_words = 0, data_bytes = 0, scratch_bytes = 0;
    // Files of one encoder repeat the same Huffman tables (27 kB per scan in device form): a scan whose tables equal those of
    // the scan before it shares that copy — one in the staging block, one upload, one set of lines in the L2.
    const host::PlannedScan::TableSet *prev_tables = nullptr;
    size_t n_table_sets = 0;
    for (uint32_t k = 0; k < n; k++) {
        if (images[k].image >= b->descs.size() || !images[k].scans || !images[k].file) return set_err(b->err, JPGPU_ERR_FORMAT, "device entropy: bad image");
        if (entry_pixels && walk_geom[images[k].image]) scratch_bytes += align_up((size_t)walk_geom[images[k].image]->mcu_h * walk_geom[images[k].image]->tiles_x * 8u, 16);
        for (const host::PlannedScan &ps : *images[k].scans) {
            if (!ps.tables) return set_err(b->err, JPGPU_ERR_FORMAT, "device entropy: scan without tables");
            if (!prev_tables || (prev_tables != ps.tables.get() && memcmp(prev_tables, ps.tables.get(), sizeof(*prev_tables)) != 0)) n_table_sets++;
            prev_tables = ps.tables.get();
            seg_words += ps.seg_off.size();
            size_t stuffed = 0;
            for (size_t sg = 0; sg + 1 < ps.seg_off.size(); sg += 2) {
                data_bytes += huff_slot_bytes(ps.seg_off[sg + 1] - ps.seg_off[sg]);
                stuffed += ps.seg_off[sg + 1] - ps.seg_off[sg];
            }
            n_sync_jobs++;  // every scan is a job of the chunk decoder, with its per-chunk state and entry buffers (device only)
            if (light && ps.check_at_staging && ps.seg_off.size() == 2) {
                n_raw_jobs++;
                const uint32_t pieces = (uint32_t)((stuffed + 15u + UNSTUFF_PIECE - 1u) / UNSTUFF_PIECE);
                max_pieces = std::max(max_pieces, pieces);
                scratch_bytes += align_up(((size_t)pieces + 1u) * 4u, 16);
                if (input_pinned) raw_scans.push_back(RawScan{images[k].file + ps.data_off, stuffed, raw_scans.size()});
            }
            if (const DriGeom g = dri_geom(ps); g.chunked) {
                const size_t chunks = g.too_large ? 0 : (size_t)(ps.seg_off.size() / 2) * g.seg_chunks;
                scratch_bytes += align_up(chunks * 8 * 4, 16) + align_up(chunks * 4, 16) + align_up(chunks * huff_emit_stride(g.shift) * 4, 16) +
                                 align_up(huff_weave_dwords((uint32_t)chunks, g.shift) * 4, 256) + 256;
            } else {  // one segment: a scan without restart markers (or one whose restart interval covers it)
                if (ps.seg_off.size() != 2 || stuffed >= (1u << 28)) return set_err(b->err, JPGPU_ERR_FORMAT, "device entropy: bad plan");
                uint32_t blocks = 0;
                for (uint32_t c = 0; c < ps.ncomp; c++) blocks += ps.comp[c].h * ps.comp[c].v;
                const uint32_t shift = huff_sync_chunk_shift((uint32_t)stuffed, blocks * ps.n_mcu, sync_blocks, sync_min_shift);
                const size_t chunks = huff_sync_chunks((uint32_t)stuffed, shift);
                scratch_bytes += align_up(chunks * 8 * 4, 16) + align_up(chunks * 4, 16) + align_up(chunks * huff_emit_stride(shift) * 4, 16) +
                                 align_up(huff_weave_dwords((uint32_t)chunks, shift) * 4, 256) + 256;
            }
        }
    }
    if (input_pinned && !raw_scans.empty()) {
        // Pinned input: files that follow one another in the caller's memory (a loader's arena) travel in ONE copy, headers and gaps
        // included; a scan's place in the mirror is then its place in the span.  Two scans share a span only if the gap between them is
        // SHORTER THAN ONE PAGE (it was 8 kB): the caller vouches for the bytes of its files only, and a gap of a page or more
        // may hold a page that is not mapped or not pinned; a gap below 4,096 bytes lies in the page of the byte in front of it and the
        // page of the byte behind it, both of which hold bytes of a file (pinning and mapping are per page).  (One
        // hipMemcpyAsync per file: 4,096 calls per call of 4,096 files — 114 ms on 16 CPUs.)  By ADDRESS, not in listing order: the
        // pipeline lists a sub-batch's images as its threads finish their headers, and an arena need not hold files in call order.
        std::sort(raw_scans.begin(), raw_scans.end(), [](const RawScan &a, const RawScan &c) { return a.src < c.src; });
        raw_mirror_off.assign(raw_scans.size(), 0);
        for (const RawScan &r : raw_scans) {
            if (spans.empty() || r.src < spans.back().end || (size_t)(r.src - spans.back().end) >= PINNED_SPAN_GAP_MAX) {
                const size_t at = spans.empty() ? 0 : align_up(spans.back().mirror_off + (size_t)(spans.back().end - spans.back().start), 16) + 16;
                spans.push_back(PinnedSpan{r.src, r.src, at});
            }
            raw_mirror_off[r.listed] = spans.back().mirror_off + (size_t)(r.src - spans.back().start);
            spans.back().end = r.src + r.bytes;
        }
    }
    const size_t off_status = 0, off_cnt = align_up(off_status + (size_t)n * 4, 16);
    const size_t off_jobs = align_up(off_cnt + n_sync_jobs * 16, 16), off_sjobs = off_jobs;
    const size_t off_ujobs = align_up(off_sjobs + n_sync_jobs * sizeof(HuffSyncJob), 16);
    const size_t off_esrc = align_up(off_ujobs + n_raw_jobs * sizeof(UnstuffJob), 16);  // entry-list pixel path: EntrySrc per BATCH image, EntryIndexJob per listed image
    const size_t off_ijobs = align_up(off_esrc + (entry_pixels ? b->descs.size() * sizeof(EntrySrc) : 0), 16);
    const size_t off_tables = align_up(off_ijobs + (entry_pixels ? (size_t)n * sizeof(EntryIndexJob) : 0), 16);
    const size_t off_seg = align_up(off_tables + n_table_sets * 8 * sizeof(DevHuffTable), 16), off_data = align_up(off_seg + seg_words * 4, 16);
    const size_t total = off_data + data_bytes;              // uploaded
    // (light: what is uploaded lands in the mirror — a copy of the data area's layout, and behind it, with pinned input, the spans)
    const size_t span_bytes = spans.empty() ? 0 : spans.back().mirror_off + (size_t)(spans.back().end - spans.back().start) + 64;
    const size_t off_mirror = align_up(total, 256), off_spans = align_up(off_mirror + data_bytes + 64, 256), dev_end = light ? off_spans + span_bytes : total;
    const size_t off_scratch = align_up(dev_end, 256), total_dev = scratch ? dev_end : off_scratch + scratch_bytes;
    if (scratch && scratch_bytes > scratch->cap) B_HIP(grow_device(scratch->d, scratch->cap, scratch_bytes));
    if (total_dev > b->entropy_cap) B_HIP(grow_device(b->d_entropy, b->entropy_cap, total_dev));
    if (total > b->entropy_host_cap) B_HIP(grow_pinned(b->h_entropy, b->entropy_host_cap, total));
    const size_t out_words = (size_t)n;
    if (out_words > b->entropy_out_cap) B_HIP(grow_pinned(b->h_entropy_out, b->entropy_out_cap, out_words, out_words + 64));
    clk.mark("buffers");
    uint8_t *h = b->h_entropy, *d = b->d_entropy;
    memset(h, 0, off_jobs);  // status words and settle counters start at zero
    HuffSyncJob *sjobs = reinterpret_cast<HuffSyncJob *>(h + off_sjobs);
    uint8_t *xs = scratch ? scratch->d : d;  // base of the device-only work space
    size_t si = 0, tcur = off_tables, tnext = off_tables, scur = off_seg, dcur = off_data, xcur = scratch ? 0 : off_scratch;
    prev_tables = nullptr;
    uint32_t max_chunks = 0;
    std::vector<uint32_t> stat_images;  // listed images, for the fills that zero their statistics
    struct CopyTask {
        uint8_t *dst;        // first slot of the scan in the pinned block
        uint32_t *seg_table; // its 2 * n_seg words
        uint32_t dst_off;    // offset of dst inside the data area (which slice of the upload the scan belongs to)
        const uint8_t *src;  // the scan's entropy-coded bytes
        const host::PlannedScan *ps;
        HuffSyncJob *sync;   // its job record (a scan of one segment: the unstuffed length goes there)
        uint32_t *h_status;  // the image's status word in the pinned block (set here if the staging pass refuses the stream)
        bool raw;            // host light: the bytes go up as they are (huff_unstuff_* does the rest on the device)
    };
    std::vector<CopyTask> copies;
    UnstuffJob *ujobs = reinterpret_cast<UnstuffJob *>(h + off_ujobs);
    size_t ui = 0;
    EntrySrc *esrc = reinterpret_cast<EntrySrc *>(h + off_esrc);
    EntryIndexJob *ijobs = reinterpret_cast<EntryIndexJob *>(h + off_ijobs);
    uint32_t n_index = 0, max_index_items = 0;
    if (entry_pixels) memset(esrc, 0, b->descs.size() * sizeof(EntrySrc));
    std::vector<std::pair<size_t, size_t>> zero_ranges;  // coefficient planes of the listed images
    b->entropy_images.clear();
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t img = images[k].image;
        b->entropy_images.push_back(img);
        const jpgpu_image_desc &desc = b->descs[img];
        bool needs_zeros = false;  // (the expansion writes every block of a scan, zeros included; planes a scan does not cover: below)
        bool image_is_light = false;
        stat_images.push_back(img);
        for (uint32_t c = 0; c < desc.ncomp; c++) {  // the class of every component: from what the expansion leaves in d_stats
            b->sane[(size_t)img * 4 + c] = 0;
            batch_class_source(b, (size_t)img * 4 + c, true);
        }
        for (const host::PlannedScan &ps : *images[k].scans) {
            // one staging task per scan: its segments, unstuffed, each in its own aligned slot (huff_stage_segment)
            const DriGeom dg = dri_geom(ps);
            HuffSyncJob *sj = &sjobs[si];
            const bool raw_scan = light && ps.check_at_staging && ps.seg_off.size() == 2;
            copies.push_back(CopyTask{h + dcur, reinterpret_cast<uint32_t *>(h + scur), (uint32_t)(dcur - off_data), images[k].file + ps.data_off, &ps, sj,
                                      reinterpret_cast<uint32_t *>(h + off_status) + k, raw_scan});
            if (raw_scan && !image_is_light) {
                image_is_light = true;
                light_images++;
            }
            size_t scan_bytes = 0, stuffed = 0;
            for (size_t sg = 0; sg + 1 < ps.seg_off.size(); sg += 2) {
                scan_bytes += huff_slot_bytes(ps.seg_off[sg + 1] - ps.seg_off[sg]);
                stuffed += ps.seg_off[sg + 1] - ps.seg_off[sg];
            }
            if (!prev_tables || (prev_tables != ps.tables.get() && memcmp(prev_tables, ps.tables.get(), sizeof(*prev_tables)) != 0)) {
                tcur = tnext;
                tnext += 8 * sizeof(DevHuffTable);
                memcpy(h + tcur, ps.tables->t, sizeof(ps.tables->t));
            }
            prev_tables = ps.tables.get();
            HuffScanComp comp[4];
            memset(comp, 0, sizeof(comp));
            uint16_t scan_q[4][64];
            memset(scan_q, 0, sizeof(scan_q));
            for (uint32_t c = 0; c < ps.ncomp; c++) {
                const uint32_t fi = ps.comp[c].frame_index;
                if (fi >= desc.ncomp || ps.comp[c].block_w != desc.components[fi].block_width)
                    return set_err(b->err, JPGPU_ERR_FORMAT, "device entropy: plan does not match the image descriptor");
                memcpy(scan_q[c], desc.quantization_tables[fi], 128);
                comp[c].dst = reinterpret_cast<int16_t *>(b->d_coef + b->coef_off[(size_t)img * 4 + fi]);
                comp[c].block_w = ps.comp[c].block_w;
                comp[c].h = ps.comp[c].h;
                comp[c].v = ps.comp[c].v;
                comp[c].dc = ps.comp[c].dc;
                comp[c].ac = ps.comp[c].ac;
                if (ps.comp[c].dc > 1u || ps.comp[c].ac > 1u) low_table_ids = false;
            }
            {
                memset(sj, 0, sizeof(*sj));
                memcpy(sj->comp, comp, sizeof(comp));
                sj->ncomp = ps.ncomp;
                memcpy(sj->q, scan_q, sizeof(scan_q));
                sj->stats = b->d_stats + (size_t)img * RS_WORDS;
                huff_sync_finish_job(*sj);
                sj->chunk_shift = dg.chunked ? dg.shift : huff_sync_chunk_shift((uint32_t)stuffed, sj->bpm * ps.n_mcu, sync_blocks, sync_min_shift);
                sj->pass0_skip = ((1u << sj->chunk_shift) >> 3) * (8u - sync_tail);
                sj->late_pass = late_pass;
                // (one segment: an upper bound, the staging task sets the real count; restart segments: slots per segment x segments)
                const uint32_t chunks = dg.chunked ? (dg.too_large ? 0u : (uint32_t)(ps.seg_off.size() / 2) * dg.seg_chunks)
                                                   : huff_sync_chunks((uint32_t)stuffed, sj->chunk_shift);
                uint32_t *st = reinterpret_cast<uint32_t *>(xs + xcur);
                // (bit positions and segment offsets are relative to the scan's first slot; light: a scan the host staged itself — restart
                // segments — lies in the mirror, where the uploads of such a launch land)
                sj->data = (light && !raw_scan) ? d + off_mirror + (dcur - off_data) : d + dcur;
                if (dg.chunked) {
                    sj->seg_off = reinterpret_cast<const uint32_t *>(d + scur);
                    sj->n_seg = (uint32_t)(ps.seg_off.size() / 2);
                    sj->ri = ps.ri;
                    sj->seg_chunks = dg.seg_chunks;
                    sj->n_chunks = chunks;
                    if (dg.too_large) reinterpret_cast<uint32_t *>(h + off_status)[k] |= 1u | 256u;  // the host decodes this image
                }
                sj->tables = reinterpret_cast<const DevHuffTable *>(d + tcur);
                sj->status = reinterpret_cast<uint32_t *>(d + off_status) + k;
                sj->changed = reinterpret_cast<uint32_t *>(d + off_cnt) + si * 4;
                sj->in_pos = st;
                sj->in_qk = st + chunks;
                sj->out_pos = st + 2 * (size_t)chunks;
                sj->out_qk = st + 3 * (size_t)chunks;
                sj->n_blocks = st + 4 * (size_t)chunks;
                sj->dc_sum = st + 5 * (size_t)chunks;
                sj->blk_end = st + 7 * (size_t)chunks;
                sj->cols = ps.cols;
                sj->n_mcu = ps.n_mcu;
                max_chunks = std::max(max_chunks, chunks);
                xcur += align_up((size_t)chunks * 8 * 4, 16);
                sj->emit_stride = huff_emit_stride(sj->chunk_shift);
                sj->emit_cnt = reinterpret_cast<uint32_t *>(xs + xcur);
                xcur += align_up((size_t)chunks * 4, 16);
                sj->emit = reinterpret_cast<uint32_t *>(xs + xcur);
                xcur += align_up((size_t)chunks * sj->emit_stride * 4, 16);
                xcur = align_up(xcur, 256);  // the weave: rows of 256 bytes (the block's base is 256-byte aligned)
                sj->weave = reinterpret_cast<const uint32_t *>(xs + xcur);
                sj->data_dwords = (uint32_t)(scan_bytes / 4);
                xcur += align_up(huff_weave_dwords(chunks, sj->chunk_shift) * 4, 256);
                if (raw_scan) {
                    UnstuffJob &uj = ujobs[ui++];
                    memset(&uj, 0, sizeof(uj));
                    // (the data area's layout in the mirror, 16-byte aligned — or the scan's place in its span: the kernels take any alignment)
                    uj.raw = input_pinned ? d + off_spans + raw_mirror_off[ui - 1u] : d + off_mirror + (dcur - off_data);
                    uj.raw_bytes = (uint32_t)stuffed;
                    uj.n_pieces = (uint32_t)((((uintptr_t)uj.raw & 15u) + stuffed + UNSTUFF_PIECE - 1u) / UNSTUFF_PIECE);
                    uj.dst = d + dcur;
                    uj.piece_kept = reinterpret_cast<uint32_t *>(xs + xcur);
                    xcur += align_up(((size_t)uj.n_pieces + 1u) * 4u, 16);
                    uj.job = reinterpret_cast<HuffSyncJob *>(d + off_sjobs) + si;
                    uj.status = sj->status;
                    sj->n_chunks = chunks;  // (an upper bound until huff_unstuff_scan_kernel has counted)
                    sj->n_bits = 0;
                }
                uint32_t block_h[4] = {0, 0, 0, 0};
                for (uint32_t c = 0; c < ps.ncomp; c++) block_h[c] = desc.components[ps.comp[c].frame_index].block_height;
                if (!huff_scan_covers_planes(*sj, block_h)) needs_zeros = true;
                // (only where the scan's MCU rows are the frame's: one interleaved scan of all components that covers the planes)
                if (const WindowGeom *kg = win_geom.empty() ? nullptr : win_geom[img]; kg && images[k].scans->size() == 1 && !needs_zeros && ps.ncomp == desc.ncomp &&
                                                                                  desc.ncomp > 1u && sj->cols == kg->mcu_w && sj->n_mcu == kg->mcu_w * kg->mcu_h) {
                    bool same = true;
                    for (uint32_t c = 0; c < ps.ncomp; c++) same = same && ps.comp[c].frame_index == c && ps.comp[c].h == kg->h[c] && ps.comp[c].v == kg->v[c];
                    if (same) window_kept_mcu_rows(*kg, sj->keep_my0, sj->keep_my1);
                }
                // Entry-list pixel path: the image's ONE scan holds its three components interleaved in frame order, 2x2 / 1x1 / 1x1, with
                // tables of their own for luma and chroma (the entries then carry their component), with or without restart segments, and
                // covers the planes of the 4:2:0 walk the image belongs to.
                if (const FusedGeom *wg = entry_pixels ? walk_geom[img] : nullptr; wg && images[k].scans->size() == 1 && !(dg.chunked && dg.too_large) && !needs_zeros &&
                                                                                    ps.ncomp == 3 && !sj->uniform && sj->bpm == 6u && sj->cols == wg->mcu_w &&
                                                                                    sj->n_mcu == wg->mcu_w * wg->mcu_h && wg->tiles_x * wg->tx >= wg->mcu_w) {
                    bool ok = true;
                    for (uint32_t c = 0; c < 3; c++) ok = ok && ps.comp[c].frame_index == c && ps.comp[c].h == (c ? 1u : 2u) && ps.comp[c].v == (c ? 1u : 2u);
                    if (ok) {
                        sj->keep_lists = 1u;
                        uint32_t *tab = reinterpret_cast<uint32_t *>(xs + xcur);
                        xcur += align_up((size_t)wg->mcu_h * wg->tiles_x * 8u, 16);
                        ijobs[n_index++] = EntryIndexJob{(uint32_t)si, wg->tx, wg->tiles_x, wg->mcu_h, tab};
                        max_index_items = std::max(max_index_items, wg->mcu_h * wg->tiles_x);
                        esrc[img] = EntrySrc{reinterpret_cast<const HuffSyncJob *>(d + off_sjobs) + si, tab};
                        b->entry_img[img] = 1;
                        b->cls_dirty = true;
                    }
                }
                si++;
            }
            dcur += scan_bytes;
            scur += ps.seg_off.size() * 4;
        }
        if (needs_zeros)
            zero_ranges.emplace_back(b->coef_off[(size_t)img * 4], b->coef_off[(size_t)img * 4 + desc.ncomp - 1] + b->coef_len[(size_t)img * 4 + desc.ncomp - 1]);
    }
    {
        hipStream_t raw_stream = (copy_stream && copy_stream != hip_stream) ? (hipStream_t)copy_stream : s;
        bool raw_copy_failed = false;
        const std::function<void(uint32_t)> body = [&](uint32_t t) {
            const CopyTask &ct = copies[t];
            if (ct.raw) {  // host light: as the file holds it — one memcpy, or none (the copy engine reads the caller's pinned buffer)
                const uint32_t nraw = ct.ps->seg_off[1] - ct.ps->seg_off[0];
                ct.seg_table[0] = 0;
                ct.seg_table[1] = nraw;  // (the stuffed length; the job's lengths come from huff_unstuff_scan_kernel)
                if (!input_pinned) copy_past_the_caches(ct.dst, ct.src + ct.ps->seg_off[0], nraw);
                return;  // (pinned input: the copy engine reads the caller's buffer — enqueued below, by this thread alone)
            }
            uint32_t o = 0;
            for (size_t sg = 0; sg + 1 < ct.ps->seg_off.size(); sg += 2) {
                const uint32_t first = ct.ps->seg_off[sg], n = ct.ps->seg_off[sg + 1] - first;
                bool clean = true;
                ct.seg_table[sg] = o;  // (relative to the scan's first slot)
                ct.seg_table[sg + 1] = huff_stage_segment(ct.dst + o, ct.src + first, n, ct.ps->check_at_staging ? &clean : nullptr);
                o += huff_slot_bytes(n);
                if (!clean) *ct.h_status |= 1u | 16u;  // something other than 0xFF00 pairs inside the scan: the host decodes this image
            }
            if (ct.sync) {
                const bool refused = (*ct.h_status & 1u) != 0u;
                if (ct.sync->n_seg > 1u) {  // restart segments in chunk slots: the slots are where they are, the segment table says what they hold
                    if (refused) ct.sync->n_chunks = 0u;
                } else {
                    ct.sync->n_bits = refused ? 0u : ct.seg_table[1] * 8u;
                    ct.sync->n_chunks = refused ? 0u : huff_sync_chunks(ct.seg_table[1], ct.sync->chunk_shift);
                }
            }
        };
        // Staging and upload in slices: while the host threads unstuff the scans of one slice into the pinned block, the
        // DMA engine carries the slice before (round 3: the whole block was staged, 2.5 ms for 256 x 1080p on the 16 CPUs the
        // box grants, and only then uploaded, 2 ms).  In front of the uploads, on the same stream, the fills: the planes start
        // as zeros (the Worker's zero-initialised plane: only non-zero coefficients are written; neighbouring images are
        // cleared with one fill — a fill per image was 1,024 tiny launches = 28 ms per 1,024 images) and so do the images' range
        // statistics.  They run while the host stages the first slice, next to nothing else of this sub-batch; on a second
        // stream (`copy_stream`) they and the uploads also stay clear of the kernels other sub-batches have in flight — behind
        // a fill on the kernels' own stream an upload waited for the machine to drain (2 of 7.5 ms per sub-batch).
        clk.mark("jobs");
        const bool two_streams = copy_stream && copy_stream != hip_stream;
        hipStream_t cps = two_streams ? (hipStream_t)copy_stream : s;
        if (two_streams && !b->entropy_uploaded) B_HIP(hipEventCreateWithFlags(&b->entropy_uploaded, hipEventDisableTiming));
        std::sort(stat_images.begin(), stat_images.end());
        for (size_t z = 0; z < stat_images.size();) {
            const size_t first = stat_images[z];
            size_t last = first;
            for (z++; z < stat_images.size() && stat_images[z] <= last + 1; z++) last = stat_images[z];
            B_HIP(hipMemsetAsync(b->d_stats + first * RS_WORDS, 0, (last - first + 1) * RS_WORDS * sizeof(uint32_t), cps));
        }
        std::sort(zero_ranges.begin(), zero_ranges.end());
        for (size_t z = 0; z < zero_ranges.size();) {
            size_t first = zero_ranges[z].first, last = zero_ranges[z].second;
            for (z++; z < zero_ranges.size() && zero_ranges[z].first <= last + 256; z++) last = std::max(last, zero_ranges[z].second);
            B_HIP(hipMemsetAsync(b->d_coef + first, 0, last - first, cps));
        }
        clk.mark("fills");
        // One parallel-for over all staging tasks; whoever finishes the last task of a slice (~8 MB of the data area) sends
        // that slice on its way.  (A parallel-for per slice spent more on starting threads than the overlap gave back.)
        const uint32_t n_tasks = (uint32_t)copies.size();
        static const uint32_t slice_shift = env_u32("JPGPU_STAGE_SLICE_SHIFT", 23, 20, 31);  // tuning knob: bytes per slice = 1 << this
        const uint32_t n_slices = std::max<uint32_t>(1u, std::min<uint32_t>({16u, n_tasks, (uint32_t)(data_bytes >> slice_shift) + 1u}));
        std::vector<std::atomic<uint32_t>> left(n_slices);
        auto slice_first = [&](uint32_t g) { return (uint32_t)((uint64_t)n_tasks * g / n_slices); };
        auto slice_of = [&](uint32_t t) {
            uint32_t g = (uint32_t)(((uint64_t)t * n_slices) / n_tasks);
            while (g + 1u < n_slices && slice_first(g + 1u) <= t) g++;
            while (g > 0u && slice_first(g) > t) g--;
            return g;
        };
        for (uint32_t g = 0; g < n_slices; g++) left[g].store(slice_first(g + 1u) - slice_first(g));
        std::atomic<int> copy_failed{0};
        std::atomic<uint32_t> max_copy_us{0}, max_task_us{0};
        const int device = b->device;
        const std::function<void(uint32_t)> staged = [&](uint32_t t) {
            const auto b0 = std::chrono::steady_clock::now();
            body(t);
            if (input_pinned && !copies[t].raw) {  // (its slots, out of the pinned block into the mirror)
                size_t bytes = 0;
                for (size_t sg = 0; sg + 1 < copies[t].ps->seg_off.size(); sg += 2) bytes += huff_slot_bytes(copies[t].ps->seg_off[sg + 1] - copies[t].ps->seg_off[sg]);
                if (hipSetDevice(device) != hipSuccess || upload_staged(d + off_mirror + copies[t].dst_off, copies[t].dst, bytes, cps) != hipSuccess) copy_failed.store(1);
            }
            if (clk.on) {
                const uint32_t us = (uint32_t)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - b0).count();
                uint32_t cur = max_task_us.load();
                while (us > cur && !max_task_us.compare_exchange_weak(cur, us)) {}
            }
            const uint32_t g = slice_of(t);
            if (left[g].fetch_sub(1u) == 1u) {  // the slice is complete
                const uint32_t t0 = slice_first(g), t1 = slice_first(g + 1u);
                const size_t lo = off_data + copies[t0].dst_off, hi = t1 < n_tasks ? off_data + copies[t1].dst_off : total;
                const auto c0 = std::chrono::steady_clock::now();
                // (light: into the mirror.  With pinned input there are no slice uploads: the raw scans have gone up on their own, straight
                // from the caller's buffers, and a slice's copy out of the pinned block would overwrite them with whatever that block
                // holds — the scans the host staged itself, restart segments, go up one by one as well: `staged` below)
                if (!input_pinned && (hipSetDevice(device) != hipSuccess || upload_staged(d + (light ? off_mirror + (lo - off_data) : lo), h + lo, hi - lo, cps) != hipSuccess))
                    copy_failed.store(1);
                if (clk.on) {
                    const uint32_t us = (uint32_t)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - c0).count();
                    uint32_t cur = max_copy_us.load();
                    while (us > cur && !max_copy_us.compare_exchange_weak(cur, us)) {}
                }
            }
        };
        if (input_pinned) {
            // one caller, one copy per span of adjacent files (4,096 hipMemcpyAsync calls from a team of sixteen threads made the call
            // twice as long as from one: 108 against 53 ms; and from one thread on 16 CPUs still 114 ms)
            for (const PinnedSpan &sp : spans)
                if (hipMemcpyAsync(d + off_spans + sp.mirror_off, sp.start, (size_t)(sp.end - sp.start), hipMemcpyHostToDevice, raw_stream) != hipSuccess) raw_copy_failed = true;
        }
        if (par && n_tasks > 1) (*par)(n_tasks, staged);
        else
            for (uint32_t t = 0; t < n_tasks; t++) staged(t);
        clk.mark("staging+uploads");
        if (clk.on) clk.used += (size_t)snprintf(clk.text + clk.used, clk.used < sizeof(clk.text) ? sizeof(clk.text) - clk.used : 0, " (slowest staging task %.2f, slowest hipMemcpyAsync call %.2f)", max_task_us.load() / 1e3, max_copy_us.load() / 1e3);
        if (copy_failed.load() || raw_copy_failed) return set_err(b->err, JPGPU_ERR_IO, "device entropy: upload of the staged scans failed");
        // the head of the block last: the staging tasks wrote into its job records (unstuffed lengths, chunk counts, status)
        B_HIP(upload_staged(d, h, off_data, cps));
        if (two_streams) {
            B_HIP(hipEventRecord(b->entropy_uploaded, cps));
            B_HIP(hipStreamWaitEvent(s, b->entropy_uploaded, 0));
        }
    }
    clk.mark("head");
    // JPGPU_BATCH_KERNEL_TIMES: events between the phases (fills | sync passes | write pass + DC sums | pixel kernels)
    static const bool phase_times = getenv("JPGPU_BATCH_KERNEL_TIMES") != nullptr;
    b->phase_events_valid = false;
    b->progressive_launch = false;
    if (phase_times) {
        for (auto &e : b->ev_phase)
            if (!e) B_HIP(hipEventCreate(&e));
        B_HIP(hipEventRecord(b->ev_phase[0], s));
    }
    if (phase_times) B_HIP(hipEventRecord(b->ev_phase[1], s));
    if (n_raw_jobs) B_HIP(launch_huff_unstuff(reinterpret_cast<const UnstuffJob *>(d + off_ujobs), (uint32_t)n_raw_jobs, max_pieces, s));
    if (n_light) *n_light = light_images;
    B_HIP(launch_huff_sync(reinterpret_cast<const HuffSyncJob *>(d + off_sjobs), (uint32_t)n_sync_jobs, max_chunks, sync_launches, sync_iters, s,
                           phase_times ? b->ev_phase[2] : nullptr, low_table_ids, reinterpret_cast<const EntryIndexJob *>(d + off_ijobs), n_index, max_index_items));
    if (n_entry) *n_entry = n_index;
    if (n_index) {
        b->entries_pending = true;
        b->d_entry_srcs = reinterpret_cast<const EntrySrc *>(d + off_esrc);
        b->d_entry_status = reinterpret_cast<const uint32_t *>(d + off_status);
        b->entry_status_n = n;
    }
    if (phase_times) {
        B_HIP(hipEventRecord(b->ev_phase[3], s));
        b->phase_events_valid = true;
    }
    clk.mark("kernels");
    // the status words into pinned memory (the only thing the host needs to look at: which images it has to decode itself)
    B_HIP(batch_status_to_host(b, reinterpret_cast<const uint32_t *>(d + off_status), n, s));
    clk.mark("status copy");
    return JPGPU_OK;
}

// JPGPU_BATCH_KERNEL_TIMES: milliseconds of the phases of the last device entropy launch and of the decode that followed it on
// the same stream ([0] fills, [1] restart-segment decoder + sync passes + block numbering, [2] write pass + DC sums,
// [3] class finalize + pixel kernels); false if they were not recorded.  The stream must have been synchronised.
bool jpgpu::batch_phase_times(jpgpu_batch *b, float ms[4]) {
    if (!b || !b->phase_events_valid) return false;
    for (int i = 0; i < 4; i++) ms[i] = 0.f;
    bool ok = hipEventElapsedTime(&ms[0], b->ev_phase[0], b->ev_phase[1]) == hipSuccess;
    ok = ok && hipEventElapsedTime(&ms[1], b->ev_phase[1], b->ev_phase[2]) == hipSuccess;
    ok = ok && hipEventElapsedTime(&ms[2], b->ev_phase[2], b->ev_phase[3]) == hipSuccess;
    if (ok && hipEventQuery(b->ev_phase[5]) == hipSuccess) ok = hipEventElapsedTime(&ms[3], b->ev_phase[4], b->ev_phase[5]) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    return ok;
}

// JPGPU_PIPE_TRACE: when the phase events of `b` fired, in milliseconds after `ref`'s first one (both recorded, streams synchronised)
bool jpgpu::batch_phase_stamps(jpgpu_batch *ref, jpgpu_batch *b, float ms[6]) {
    if (!ref || !b || !ref->phase_events_valid || !b->phase_events_valid) return false;
    bool ok = true;
    for (int i = 0; i < 6 && ok; i++) {
        ms[i] = -1.f;
        if (hipEventQuery(b->ev_phase[i]) == hipSuccess) ok = hipEventElapsedTime(&ms[i], ref->ev_phase[0], b->ev_phase[i]) == hipSuccess;
    }
    if (!ok) (void)hipGetLastError();
    return ok;
}

// ---- progressive frames on the device (huff_prog_wave.hpp) ------------------------------------------------------------------------
// Staging block (same offsets in the pinned and the device copy):
//   [ status: n x u32 | ProgTrack[] | ProgScan[] | ProgHuffTable[] | scan bytes ]     device only: the masks (16 bytes per block)
int jpgpu::batch_device_progressive_launch(jpgpu_batch *b, const DeviceProgressiveImage *images, uint32_t n, void *hip_stream,
                                           const std::function<void(uint32_t, const std::function<void(uint32_t)> &)> *par, void *copy_stream,
                                           DeviceScratch *scratch, bool allow_pipelined) {
    if (!b || !images || n == 0) return JPGPU_ERR_FORMAT;
    int rc = use_device(b->device, b->err);
    if (rc) return rc;
    if (!b->d_coef) return set_err(b->err, JPGPU_ERR_FORMAT, "batch has no device buffers bound");
    if (n != b->descs.size()) return set_err(b->err, JPGPU_ERR_FORMAT, "device progressive: every image of the batch must be listed");
    hipStream_t s = (hipStream_t)hip_stream;
    rc = batch_enable_dev_classes(b);
    if (rc) return rc;
    batch_drop_entries(b);  // (the frames' coefficients go to the arena: a sub-batch reused after an entry-list call must not skip them)
    size_t n_scans = 0, n_tracks = 0, n_tables = 0, data_bytes = 0, mask_bytes = 0;
    for (uint32_t k = 0; k < n; k++) {
        if (images[k].image >= b->descs.size() || !images[k].plan || !images[k].file) return set_err(b->err, JPGPU_ERR_FORMAT, "device progressive: bad image");
        const host::ProgPlan &pl = *images[k].plan;
        n_scans += pl.scans.size();
        n_tracks += pl.n_tracks;
        for (const host::ProgPlannedScan &ps : pl.scans) {
            for (int t = 0; t < 4; t++)
                if (ps.table[t]) n_tables++;
            data_bytes += huff_slot_bytes(ps.stuffed_bytes);
        }
        const jpgpu_image_desc &desc = b->descs[images[k].image];
        for (uint32_t c = 0; c < desc.ncomp; c++) mask_bytes += align_up(b->coef_len[(size_t)images[k].image * 4 + c] / 128 * 16, 256);
    }
    // One WAVE per scan (huff_prog_wave.hpp), the scans of a track pipelined (huff_prog_job.hpp): a progress word each (behind the masks,
    // zeroed with them); the launch order below keeps a frame's waves on one XCD, producers in front, so an oversubscribed launch
    // cannot starve a producer.  JPGPU_PROG_SERIAL=1 / !allow_pipelined (tests): a wave per TRACK, its scans one after the other.
    // (Round 5 walked a LANE per scan — huff_prog_core.hpp, in the git history: 3 x slower at 256 frames, 25 % at 4,096 distinct ones.)
    static const bool serial_env = getenv("JPGPU_PROG_SERIAL") != nullptr;
    const bool serial_tracks = serial_env || !allow_pipelined;
    const size_t progress_off = mask_bytes;
    mask_bytes += align_up(n_scans * 4u, 256);
    // (eight lists that differ by less than one frame's 256 scans)
    const size_t max_lanes = n_tracks + n_scans + 64u * 64u;
    n_tracks = max_lanes;
    const size_t off_status = 0, off_tracks = align_up((size_t)n * 4, 16), off_scans = align_up(off_tracks + n_tracks * sizeof(ProgTrack), 16);
    const size_t off_tables = align_up(off_scans + n_scans * sizeof(ProgScan), 16), off_data = align_up(off_tables + n_tables * sizeof(ProgHuffTable), 16);
    const size_t total = off_data + data_bytes;
    const size_t off_masks = align_up(total, 256), total_dev = scratch ? total : off_masks + mask_bytes;
    if (scratch && mask_bytes > scratch->cap) B_HIP(grow_device(scratch->d, scratch->cap, mask_bytes));
    if (total_dev > b->entropy_cap) B_HIP(grow_device(b->d_entropy, b->entropy_cap, total_dev));
    if (total > b->entropy_host_cap) B_HIP(grow_pinned(b->h_entropy, b->entropy_host_cap, total));
    if ((size_t)n > b->entropy_out_cap) B_HIP(grow_pinned(b->h_entropy_out, b->entropy_out_cap, (size_t)n, (size_t)n + 64));
    uint8_t *h = b->h_entropy, *d = b->d_entropy, *dm = scratch ? scratch->d : d + off_masks;
    memset(h, 0, off_tracks);  // status words
    ProgTrack *tracks = reinterpret_cast<ProgTrack *>(h + off_tracks);
    ProgScan *scans = reinterpret_cast<ProgScan *>(h + off_scans);
    struct StageTask {
        const host::ProgPlannedScan *ps;
        const uint8_t *src;
        uint8_t *dst;       // the scan's slot in the pinned block
        uint8_t *tables;    // where its tables go in the pinned block
        ProgScan *scan;
        uint32_t *h_status;
    };
    std::vector<StageTask> tasks;
    tasks.reserve(n_scans);
    struct TrackOrder {
        uint32_t first_scan, n_scans, image_k;
        uint64_t weight;  // bytes of entropy-coded data the lane walks
        uint32_t rank;    // pipelined scans: how many scans deep its dependencies go (0: none); serial tracks: 0
        uint32_t kind;    // pipelined scans: which scan of its frame's script it is (band, approximation, first component); serial tracks: 0
        uint64_t chain;   // pipelined scans: the place of this scan's track among its frame's tracks by the bytes along the longest chain of dependent scans (0: the longest; waves: the launch order)
    };
    std::vector<TrackOrder> order;
    order.reserve(n_tracks);
    size_t si = 0, tcur = off_tables, dcur = off_data, mcur = 0;
    b->entropy_images.clear();
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t img = images[k].image;
        b->entropy_images.push_back(img);
        const jpgpu_image_desc &desc = b->descs[img];
        const host::ProgPlan &pl = *images[k].plan;
        uint64_t *mask_of[4] = {nullptr, nullptr, nullptr, nullptr};
        for (uint32_t c = 0; c < desc.ncomp; c++) {
            mask_of[c] = reinterpret_cast<uint64_t *>(dm + mcur);
            mcur += align_up(b->coef_len[(size_t)img * 4 + c] / 128 * 16, 256);
        }
        // Which scans does a scan depend on?  For every coefficient it covers, the LAST earlier scan that covered it (that one waited
        // for its own predecessors block by block, so staying behind it is staying behind them all).  More than three, or more than
        // 64 levels: the frame's tracks are walked serially, one lane each.
        const size_t first_si = si;
        const uint32_t ns = (uint32_t)pl.scans.size();
        const host::ProgDependencies pd = serial_tracks ? host::ProgDependencies{} : host::prog_plan_dependencies(pl);
        const bool pipelined = !serial_tracks && pd.ok;
        const std::vector<uint32_t> &rank = pd.rank;
        const std::vector<std::array<int32_t, 3>> &deps = pd.deps;
        // the scans, in stream order (serial tracks: grouped by track, each track's scans contiguous)
        std::vector<uint32_t> scan_order;
        if (pipelined) {
            for (uint32_t j = 0; j < ns; j++) scan_order.push_back(j);
        } else {
            for (uint32_t t = 0; t < pl.n_tracks; t++)
                for (uint32_t j = 0; j < ns; j++)
                    if (pl.scans[j].track == t) scan_order.push_back(j);
        }
        std::vector<size_t> si_of(ns, 0);
        for (uint32_t j : scan_order) {
            const host::ProgPlannedScan &ps = pl.scans[j];
            ProgScan &sc = scans[si];
            si_of[j] = si;
            memset(&sc, 0, sizeof(sc));
            sc.data = d + dcur;
            sc.ss = ps.ss, sc.se = ps.se, sc.ah = ps.ah, sc.al = ps.al;
            sc.ncomp = ps.ncomp, sc.cols = ps.cols, sc.rows = ps.rows;
            for (uint32_t c = 0; c < ps.ncomp; c++) {
                const uint32_t fi = ps.comp[c].frame_index;
                if (fi >= desc.ncomp || ps.comp[c].block_w != desc.components[fi].block_width)
                    return set_err(b->err, JPGPU_ERR_FORMAT, "device progressive: plan does not match the image descriptor");
                sc.comp[c].coefs = reinterpret_cast<int16_t *>(b->d_coef + b->coef_off[(size_t)img * 4 + fi]);
                sc.comp[c].masks = mask_of[fi];
                sc.comp[c].block_w = ps.comp[c].block_w;
                sc.comp[c].h = ps.comp[c].h;
                sc.comp[c].v = ps.comp[c].v;
                sc.comp[c].table = ps.comp[c].table;
            }
            StageTask st{&ps, images[k].file + ps.data_off, h + dcur, h + tcur, &sc, reinterpret_cast<uint32_t *>(h + off_status) + k};
            for (int tb = 0; tb < 4; tb++)
                if (ps.table[tb]) {
                    sc.table[tb] = reinterpret_cast<const ProgHuffTable *>(d + tcur);
                    tcur += sizeof(ProgHuffTable);
                }
            tasks.push_back(st);
            dcur += huff_slot_bytes(ps.stuffed_bytes);
            si++;
        }
        if (pipelined) {
            for (uint32_t j = 0; j < ns; j++) {
                ProgScan &sc = scans[si_of[j]];
                sc.progress = reinterpret_cast<uint32_t *>(dm + progress_off) + si_of[j];
                for (uint32_t w = 0; w < 3u; w++) {
                    if (deps[j][w] < 0) continue;
                    sc.wait[w] = reinterpret_cast<const uint32_t *>(dm + progress_off) + si_of[(uint32_t)deps[j][w]];
                    if (!host::prog_same_walk(pl.scans[j], pl.scans[(uint32_t)deps[j][w]])) sc.wait_whole |= 1u << w;  // (else block for block)
                }
                const host::ProgPlannedScan &pj = pl.scans[j];
                const uint32_t kind = ((uint32_t)pj.ss << 24) | ((uint32_t)pj.se << 16) | ((uint32_t)pj.ah << 12) | ((uint32_t)pj.al << 8) | (pj.comp[0].frame_index << 4) | pj.ncomp;
                order.push_back(TrackOrder{(uint32_t)si_of[j], 1u, k, pj.stuffed_bytes, rank[j], kind, 0u});
            }
            {   // the longest chain of every track: a scan's bytes + the longest chain of the scans that wait for it, the maximum per track
                std::vector<uint64_t> down(ns, 0u), best(pl.n_tracks + 1u, 0u);
                for (uint32_t j = ns; j-- > 0;) {  // (consumers come later in the stream: down[j] is final when the loop reaches j)
                    down[j] += pl.scans[j].stuffed_bytes;
                    for (uint32_t w = 0; w < 3u; w++)
                        if (deps[j][w] >= 0) down[(uint32_t)deps[j][w]] = std::max(down[(uint32_t)deps[j][w]], down[j]);
                }
                for (uint32_t j = 0; j < ns; j++) {
                    uint64_t &bt = best[std::min<uint32_t>(pl.scans[j].track, pl.n_tracks)];
                    bt = std::max(bt, down[j]);
                }
                // ... as the track's PLACE among the frame's tracks (0: the longest chain): frames differ in their bytes, the places compare
                for (uint32_t j = 0; j < ns; j++) {
                    const uint64_t mine = best[std::min<uint32_t>(pl.scans[j].track, pl.n_tracks)];
                    uint32_t place = 0;
                    for (uint32_t t = 0; t < pl.n_tracks; t++)
                        if (best[t] > mine || (best[t] == mine && t < std::min<uint32_t>(pl.scans[j].track, pl.n_tracks))) place++;
                    order[order.size() - ns + j].chain = place;
                }
            }
        } else {
            size_t at = first_si;
            for (uint32_t t = 0; t < pl.n_tracks; t++) {
                TrackOrder to{(uint32_t)at, 0u, k, 0u, 0u, 0u, 0u};
                for (uint32_t j = 0; j < ns; j++)
                    if (pl.scans[j].track == t) {
                        to.weight += pl.scans[j].stuffed_bytes;
                        to.n_scans++;
                    }
                at += to.n_scans;
                if (to.n_scans) order.push_back(to);
            }
        }
        for (uint32_t c = 0; c < desc.ncomp; c++) {  // the classes of the finished planes: from the range scan below
            b->sane[(size_t)img * 4 + c] = 0;
            batch_class_source(b, (size_t)img * 4 + c, true);
        }
    }
    // Lanes in launch order: by dependency rank (producers in front: workgroups are dispatched in order, so whatever a lane waits for is
    // resident or done), every rank starting a wave of its own (a lane never waits for a lane of its own wave), and inside a rank like
    // with like — the same scan of the frames' scripts side by side (a wave whose lanes walk DC, first AC and refinement scans runs the
    // three loops one after the other), heavy lanes first: the 64 lanes of a wave walk scans of the same kind and about the same length
    std::stable_sort(order.begin(), order.end(), [](const TrackOrder &a, const TrackOrder &c) {
        return a.rank != c.rank ? a.rank < c.rank : (a.kind != c.kind ? a.kind < c.kind : a.weight > c.weight);
    });
    size_t n_lanes = 0;
    const auto entry_of = [&](const TrackOrder &o) {
        return ProgTrack{reinterpret_cast<const ProgScan *>(d + off_scans) + o.first_scan, o.n_scans, reinterpret_cast<uint32_t *>(d + off_status) + o.image_k};
    };
    {
        // Waves in launch order (huff.hip, huff_progw_kernel): workgroup i runs on XCD i mod 8 and every XCD dispatches its workgroups in
        // order.  So: every frame's waves on ONE XCD (the frame with the fewest waves so far takes the next frame: lists of equal length),
        // and inside an XCD's list by dependency rank, in groups of JPGPU_PROG_GROUP frames (default: all — rank-major: the waves of a
        // rank run at full occupancy before the next rank's are dispatched; a wave that catches up with its producer sleeps), inside a
        // rank the heavy scans first.  A producer is in front of its consumers in the list of their XCD: when a consumer runs, the
        // producer is resident or done — no deadlock however many waves the launch has, and a frame's planes and masks stay in one L2.
        static const uint32_t group = getenv("JPGPU_PROG_GROUP") ? (uint32_t)std::max(1, atoi(getenv("JPGPU_PROG_GROUP"))) : 0x7fffffffu;
        constexpr uint32_t XCDS = 8u;
        std::vector<uint32_t> xcd_of(n, 0u), seq_of(n, 0u);  // per listed image: its XCD, its number among that XCD's frames
        {
            std::vector<uint32_t> per_image(n, 0u);
            for (const TrackOrder &o : order) per_image[o.image_k]++;
            size_t load[XCDS] = {0, 0, 0, 0, 0, 0, 0, 0};
            uint32_t frames[XCDS] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (uint32_t k = 0; k < n; k++) {
                uint32_t x = 0;
                for (uint32_t j = 1; j < XCDS; j++)
                    if (load[j] < load[x]) x = j;
                xcd_of[k] = x;
                seq_of[k] = frames[x]++;
                load[x] += per_image[k];
            }
        }
        std::vector<TrackOrder> lists[XCDS];
        for (const TrackOrder &o : order) lists[xcd_of[o.image_k]].push_back(o);
        size_t longest = 0;
        for (auto &l : lists) {
            // (round 6, second half: the tracks with the longest chains FIRST — Y's first scans, their refinements, then the short tracks:
            // with ranks only, the last scans of the long chains were dispatched last and the launch ended with a 9 ms tail of a few
            // waves per SIMD; scans of one track share `chain`, and inside a track the rank keeps producers in front.  JPGPU_PROG_ORDER=rank: as before)
            static const bool by_rank = getenv("JPGPU_PROG_ORDER") && !strcmp(getenv("JPGPU_PROG_ORDER"), "rank");
            std::stable_sort(l.begin(), l.end(), [&](const TrackOrder &a, const TrackOrder &c) {
                const uint32_t ga = seq_of[a.image_k] / group, gc = seq_of[c.image_k] / group;
                if (ga != gc) return ga < gc;
                if (!by_rank && a.chain != c.chain) return a.chain < c.chain;
                return a.rank != c.rank ? a.rank < c.rank : a.weight > c.weight;
            });
            longest = std::max(longest, l.size());
        }
        if (longest * XCDS > max_lanes) return set_err(b->err, JPGPU_ERR_INTERNAL, "device progressive: wave table");
        for (size_t j = 0; j < longest; j++)
            for (uint32_t x = 0; x < XCDS; x++) tracks[n_lanes++] = j < lists[x].size() ? entry_of(lists[x][j]) : ProgTrack{nullptr, 0u, nullptr};
    }
    const bool two_streams = copy_stream && copy_stream != hip_stream;
    hipStream_t cps = two_streams ? (hipStream_t)copy_stream : s;
    if (two_streams && !b->entropy_uploaded) B_HIP(hipEventCreateWithFlags(&b->entropy_uploaded, hipEventDisableTiming));
    // zeros: the planes (the Worker's zero-initialised plane: src/decoder.rs:400-412), the masks, the statistics
    // (the masks on the kernels' own stream: with a caller's `scratch` they are shared by the launches of that stream, which run one
    // after the other there — a fill on the copy stream would run into the previous launch's walk)
    B_HIP(hipMemsetAsync(b->d_coef, 0, b->coef_bytes, cps));
    B_HIP(hipMemsetAsync(dm, 0, mask_bytes, s));
    const std::function<void(uint32_t)> stage = [&](uint32_t t) {
        const StageTask &st = tasks[t];
        bool clean = true;
        st.scan->n_bytes = huff_stage_segment(st.dst, st.src, st.ps->stuffed_bytes, &clean);
        if (!clean) *st.h_status |= PROG_ST_HOST | PROG_ST_STAGING;  // (cannot happen: the planner walked the same bytes)
        uint8_t *tp = st.tables;
        for (int tb = 0; tb < 4; tb++)
            if (st.ps->table[tb]) {
                memcpy(tp, st.ps->table[tb].get(), sizeof(ProgHuffTable));
                tp += sizeof(ProgHuffTable);
            }
    };
    if (par && tasks.size() > 1) (*par)((uint32_t)tasks.size(), stage);
    else
        for (uint32_t t = 0; t < tasks.size(); t++) stage(t);
    B_HIP(upload_staged(d, h, total, cps));
    if (two_streams) {
        B_HIP(hipEventRecord(b->entropy_uploaded, cps));
        B_HIP(hipStreamWaitEvent(s, b->entropy_uploaded, 0));
    }
    // events around the track kernel: always (the pipeline's dispatcher learns the device's latency from them), and the phase events of
    // JPGPU_BATCH_KERNEL_TIMES ([1]..[2] "sync" = the track kernel, [2]..[3] "write" = the range scan)
    for (auto &e : b->ev_phase)
        if (!e) B_HIP(hipEventCreate(&e));
    B_HIP(hipEventRecord(b->ev_phase[0], s));
    B_HIP(hipEventRecord(b->ev_phase[1], s));
    B_HIP(launch_huff_progw(reinterpret_cast<const ProgTrack *>(d + off_tracks), (uint32_t)n_lanes, s));
    B_HIP(hipEventRecord(b->ev_phase[2], s));
    if (getenv("JPGPU_PROG_TIMES")) {  // (debugging aid: a synchronisation inside the launch)
        B_HIP(hipStreamSynchronize(s));
        const uint32_t ns = (uint32_t)images[0].plan->scans.size();
        std::vector<ProgScan> back(ns);
        B_HIP(hipMemcpy(back.data(), d + off_scans, ns * sizeof(ProgScan), hipMemcpyDeviceToHost));
        for (uint32_t j = 0; j < ns; j++)
            fprintf(stderr, "prog times: frame 0 scan %u (ss %u se %u ah %u al %u, %u bytes): %.3f ms\n", j, back[j].ss, back[j].se, back[j].ah, back[j].al, back[j].n_bytes, back[j].report[0] * 1e-5);
        for (uint32_t j = 0; j < ns; j++)
            if (back[j].ah && back[j].ss) fprintf(stderr, "prog times: frame 0 scan %u: %u calls of the hand-scheduled loop, %u symbols on the portable path, %u window switches\n", j, back[j].report[1], back[j].report[2], back[j].report[3]);
    }
    {
        const int crc = jpgpu_batch_classify_on_device(b, s);
        if (crc) return crc;
    }
    B_HIP(hipEventRecord(b->ev_phase[3], s));
    b->phase_events_valid = true;
    b->progressive_launch = true;
    B_HIP(batch_status_to_host(b, reinterpret_cast<const uint32_t *>(d + off_status), n, s));
    return JPGPU_OK;
}

bool jpgpu::batch_progressive_kernel_ms(jpgpu_batch *b, float *ms) {
    if (!b || !ms || !b->progressive_launch || !b->ev_phase[1] || !b->ev_phase[2]) return false;
    if (hipEventElapsedTime(ms, b->ev_phase[1], b->ev_phase[2]) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return true;
}

int jpgpu::batch_device_entropy_collect(jpgpu_batch *b, uint32_t *status, uint32_t n) {
    if (!b || !status || n != b->entropy_images.size()) return JPGPU_ERR_FORMAT;
    // (the classes of the accepted images stay on the device: d_stats; an image the host decodes instead gets its class with
    // its upload)
    for (uint32_t k = 0; k < n; k++) status[k] = b->h_entropy_out[k];
    b->entropy_images.clear();
    return JPGPU_OK;
}
