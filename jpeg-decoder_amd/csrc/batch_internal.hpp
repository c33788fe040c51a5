// batch_internal.hpp — struct jpgpu_batch and the helpers that batch.cpp (creation, job tables, decode), batch_output.cpp (the
// fixed-output stage) and batch_entropy.cpp (the device entropy and progressive launches) share.  Internal to those translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "batch_layout.hpp"
#include "batch_output.hpp"
#include "compact.hpp"
#include "fused.hpp"
#include "fused_entries.hpp"
#include "fused_scaled.hpp"
#include "host_common.hpp"
#include "huff.hpp"
#include "kernels.hpp"
#include "range_stats.hpp"
#include "window_band.hpp"

using namespace jpgpu;

// A launch group of a band kernel (fused_scaled.hpp, window_band.hpp): its images, their geometries and job tables on the host and
// on the device, and the launch's extents.  PlaneJobs carry the coefficient / table pointers (no u8 planes in HBM: the kernels keep
// them in LDS), ImageJobs the upsampler kinds and the output; Geom::first_plane_job indexes the launch's PlaneJob table.
template <typename Geom>
struct BandGroup {
    std::vector<uint32_t> ids;  // in image order
    std::vector<Geom> geoms;
    std::vector<PlaneJob> plane_jobs;
    std::vector<ImageJob> image_jobs;
    Geom *d_geoms = nullptr;
    PlaneJob *d_plane_jobs = nullptr;
    ImageJob *d_image_jobs = nullptr;
    uint32_t max_tiles_x = 0, max_bands = 0, lds_bytes = 0;
    bool scales[9] = {false, false, false, false, false, false, false, false, false};

    bool empty() const { return ids.empty(); }
    void add(uint32_t image, const Geom &g) {
        ids.push_back(image);
        geoms.push_back(g);
        extend(g);
    }
    void extend(const Geom &g) {
        max_tiles_x = std::max(max_tiles_x, g.tiles_x);
        max_bands = std::max(max_bands, g.bands);
        lds_bytes = std::max(lds_bytes, g.lds_bytes);
        scales[g.scale] = true;
    }
    // after the last add: the PlaneJob numbering, the device tables, the geometries' upload
    hipError_t number_and_alloc(const std::vector<jpgpu_image_desc> &descs) {
        if (ids.empty()) return hipSuccess;
        hipError_t e = hipMalloc((void **)&d_geoms, ids.size() * sizeof(Geom));
        if (e == hipSuccess) e = hipMalloc((void **)&d_plane_jobs, ids.size() * 4 * sizeof(PlaneJob));
        if (e == hipSuccess) e = hipMalloc((void **)&d_image_jobs, ids.size() * sizeof(ImageJob));
        return e == hipSuccess ? set_geoms(geoms, descs) : e;
    }
    // other geometries for the same images (batch_rewindow): numbering, extents, upload
    hipError_t set_geoms(const std::vector<Geom> &g, const std::vector<jpgpu_image_desc> &descs) {
        geoms = g;
        max_tiles_x = max_bands = lds_bytes = 0;
        for (bool &s : scales) s = false;
        uint32_t pj = 0;
        for (size_t k = 0; k < ids.size(); k++) {
            geoms[k].first_plane_job = pj;
            pj += descs[ids[k]].ncomp;
            extend(geoms[k]);
        }
        return hipMemcpy(d_geoms, geoms.data(), geoms.size() * sizeof(Geom), hipMemcpyHostToDevice);
    }
    int fill_jobs(jpgpu_batch *b, uint8_t *pix, const std::vector<size_t> &pix_off);  // the job tables, built and uploaded
    void free() {
        if (d_geoms) (void)hipFree(d_geoms);
        if (d_plane_jobs) (void)hipFree(d_plane_jobs);
        if (d_image_jobs) (void)hipFree(d_image_jobs);
    }
};

// The fixed-output stage of a batch (batch_output.hpp: the options, the rules, the route; batch_output.cpp: the code).  With an output size
// the output arena (d_out, out_off, out_len, out_bytes) holds h x w x channels elements per image, and every pixel kernel writes what it
// always writes — the window's or the whole image's pixels — into an intermediate arena the batch owns (d_pix), which the route's resample
// launch reads.  `d_jobs` holds the route's device records: ResampleJobs or TensorJobs (2 n: [0, n) for the band launch, [n, 2 n) the real
// jobs of the images whose bands go in runs — bpr[i] != 0, the band launch sees such an image with no band), PlacedJobs or
// PlacedTensorJobs (n: `jobs[i]` is then the job of image i's visible rectangle, places[i] where it lies).  Tensor records, and a warp's
// WarpJobs with the N-sep tables behind them ([n WarpJob | n x (w + h) int32]), travel from pinned mirrors on the decode's stream: fresh
// flips and matrices come with every call of a loader.  A warp reads a second arena (d_wsrc), which the u8 resample then writes.
// Orientations: a launch in front of the resample and an arena of its own, at the struct's end.
struct OutputStage {
    OutputSpec spec;
    OutputRoute route;
    std::vector<size_t> pix_off, pix_len, wsrc_off;  // the intermediate arena, the warp's source arena
    size_t pix_bytes = 0, pix_cap = 0;
    uint8_t *d_pix = nullptr, *d_wsrc = nullptr;
    std::vector<ResampleJob> jobs;  // per image
    std::vector<int32_t> tab;       // the images' tables (equal axes share one)
    std::vector<uint32_t> bpr;      // per image: bands per run (0: the image keeps its bands)
    int32_t *d_tab = nullptr;
    size_t tab_cap = 0;             // int32 words behind d_tab
    uint32_t *d_bpr = nullptr;
    void *d_tn_table = nullptr;     // 4 x 256 elements
    uint32_t max_bands = 0, max_runs = 0, lds_bytes = 0;  // (max_bands over the images that keep their bands, max_runs over the others)
    bool placed = false;            // for the batch's lifetime: other device records, another launch
    std::vector<jpgpu_placement> pl;  // per image, normalised (normalise_placements)
    std::vector<Place> places;        // per image
    void *d_jobs = nullptr, *h_jobs = nullptr;
    uint8_t *d_wp_jobs = nullptr, *h_wp_jobs = nullptr;
    hipEvent_t tn_sent = nullptr, wp_sent = nullptr;  // behind the last copy out of each mirror
    std::vector<uint8_t> flips;    // per image (jpgpu_batch_set_flips)
    std::vector<jpgpu_warp> m;     // per image (jpgpu_batch_set_warps)
    bool tn_dirty = false, wp_dirty = false;  // flips / matrices changed: the records go up before the next decode
    // Orientations (route.orient; orient_band.hpp): orient[i] per image for the batch's lifetime.  The images with another value than 1
    // (or_ids, in image order) have a job each in or_jobs, which rewrites the image's pixels in d_pix, oriented, into d_or at
    // or_off[image] — where the image's resample job then reads.  output_retable lays the arena out, for these images alone.
    std::vector<uint8_t> orient;
    std::vector<uint32_t> or_ids;
    std::vector<size_t> or_off;
    std::vector<OrientJob> or_jobs;
    uint8_t *d_or = nullptr;
    size_t or_cap = 0;
    OrientJob *d_or_jobs = nullptr;
    uint32_t or_max_tiles = 0;
    // Colour (route.colour; colour_band.hpp): every image's program (jpgpu_batch_set_colour_programs), built into ColourJobs in a pinned
    // mirror and sent on the decode's stream like the WarpJobs; the launch rewrites the warp's source arena in place, between the u8
    // resample and the warp launch.  d_cl_scale: colour_scale_table.
    std::vector<ColourProgram> programs;
    ColourJob *d_cl_jobs = nullptr, *h_cl_jobs = nullptr;
    double *d_cl_scale = nullptr;
    hipEvent_t cl_sent = nullptr;
    bool cl_dirty = false;
    void free() {
        for (void *d : {(void *)d_pix, (void *)d_wsrc, (void *)d_tab, (void *)d_bpr, d_tn_table, d_jobs, (void *)d_wp_jobs, (void *)d_or, (void *)d_or_jobs,
                        (void *)d_cl_jobs, (void *)d_cl_scale})
            if (d) (void)hipFree(d);
        if (h_jobs) (void)hipHostFree(h_jobs);
        if (h_wp_jobs) (void)hipHostFree(h_wp_jobs);
        if (h_cl_jobs) (void)hipHostFree(h_cl_jobs);
        if (tn_sent) (void)hipEventDestroy(tn_sent);
        if (wp_sent) (void)hipEventDestroy(wp_sent);
        if (cl_sent) (void)hipEventDestroy(cl_sent);
    }
};
// batch_output.cpp, what batch.cpp calls: at creation, on a refresh of the job tables, on a decode behind the pixel kernels, and for
// other windows or placements (also the last step of creation).
int output_create(jpgpu_batch *b);
int output_bind(jpgpu_batch *b, hipStream_t stream, bool all);
int output_launch(jpgpu_batch *b, hipStream_t s);
int output_retable(jpgpu_batch *b);

struct jpgpu_batch {
    int device = 0;
    uint32_t flags = 0;
    std::string err;
    std::string path = "generic";
    std::vector<jpgpu_image_desc> descs;
    // arena layout
    std::vector<size_t> coef_off;   // [image*4 + comp]
    std::vector<size_t> coef_len;   // bytes
    std::vector<size_t> plane_off;  // [image*4 + comp] (generic path scratch)
    std::vector<size_t> out_off, out_len;
    std::vector<size_t> out_full_len;  // per image: bytes of its whole output (out_len of an image without a window)
    size_t out_cap = 0;                // bytes allocated behind d_out (own_out; >= out_bytes: batch_rewindow)
    size_t coef_bytes = 0, out_bytes = 0, plane_bytes_total = 0;
    uint8_t *d_coef = nullptr, *d_out = nullptr;
    bool own_coef = false, own_out = false;
    uint8_t *d_planes = nullptr;
    uint16_t *d_qt = nullptr;
    PlaneJob *d_plane_jobs = nullptr;
    ImageJob *d_image_jobs = nullptr;
    std::vector<PlaneJob> plane_jobs;
    std::vector<ImageJob> image_jobs;
    std::vector<uint8_t> sane;  // per image*4+comp: 1 if every |c*q| < 2^15 (24-bit path exact)
    uint32_t max_blocks = 0, max_w = 0, max_h = 0;
    bool scales[9] = {false, false, false, false, false, false, false, false, false};
    bool jobs_dirty = true;
    bool qt_dirty = false;
    std::vector<FusedPlan> fused;       // one per fusable kind present in the batch
    std::vector<uint32_t> generic_ids;  // images on the generic path
    // Reduced-size decodes in one launch (fused_scaled.hpp): images whose components all sit at one dct_scale < 8 — their own job
    // tables (PlaneJobs carry the coefficient / table pointers, ImageJobs the upsampler kinds and the output), no u8 planes in HBM
    BandGroup<ScaledGeom> scaled;
    std::string scaled_name;            // path name of the scaled launch group ("fused420-s4", ...; "fusedscaled-mixed")
    // Windows (jpgpu_batch_create_windowed, window_band.hpp): images with a window smaller than the image form a group of their own —
    // never in a fused plan, the scaled or the generic group.  Their coefficients are whole-image arena entries as ever, their output
    // is the window's bytes; the kernel works with exact arithmetic at every scale, so their range classes play no part.
    BandGroup<WindowGeom> win;
    OutputStage o;  // a fixed output size and what follows it (o.spec.w == 0: none)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // Behind the last work enqueued on a caller's stream that reads the batch's tables or its coefficient arena (every decode,
    // jpgpu_batch_classify_on_device).  That stream may be a non-blocking one, which a blocking copy on the null stream does not order
    // against: every host-side rewrite of something such work reads waits for the event first (batch_wait_enqueued) — only then, so a
    // decode after a decode with nothing changed never waits.
    hipEvent_t enqueued = nullptr;
    bool enqueue_pending = false;
    // compact transport (compact.hpp): staging area in HBM, allocated at the first jpgpu_batch_upload_compact
    std::mutex compact_mutex;
    uint8_t *d_compact = nullptr;
    std::vector<size_t> compact_off;      // [image*4 + comp]
    std::vector<uint8_t> compact_pending; // [image*4 + comp]: uploaded, to be expanded by the next decode
    ExpandJob *d_expand_jobs = nullptr;
    ExpandJob *h_expand_jobs = nullptr;   // pinned mirror: the jobs travel on the decode's stream, behind the expansion before them
    hipEvent_t expand_sent = nullptr;     // behind the last copy out of the mirror
    bool any_compact_pending = false;
    // device entropy decoding (huff.hip): one pinned + one device staging block, grown on demand
    uint8_t *h_entropy = nullptr, *d_entropy = nullptr;
    size_t entropy_cap = 0, entropy_host_cap = 0;
    uint32_t *h_entropy_out = nullptr;  // pinned read-back: status per listed image, then 2 range stats per (image, comp)
    size_t entropy_out_cap = 0;
    hipEvent_t entropy_uploaded = nullptr, entropy_filled = nullptr;
    uint8_t *d_scan = nullptr;     // jpgpu_batch_scan_ranges: stats + job table on the device, kept between calls
    uint32_t *h_scan = nullptr;    // pinned read-back of the stats
    size_t scan_cap = 0;
    bool scan_jobs_valid = false;  // the job table on the device matches the bound arena and the current q-tables
    uint8_t *h_bounce = nullptr;  // pinned: jpgpu_batch_download into pageable memory
    size_t h_bounce_cap = 0;
    std::vector<uint32_t> entropy_images;  // images of the launch in flight
    size_t entropy_out_off = 0;            // offset of the status / stats words inside d_entropy
    // Classes decided ON THE DEVICE (range_stats.hpp): statistics raised by the kernels that write the coefficients, turned
    // into class bits by class_finalize_* in front of the pixel kernels.  cls_src[image * 4 + comp] = 1: that component's
    // class comes from the image's statistics; 0: from `sane` (what the host knows).  dev_classes: some component does, so
    // decodes run the finalize kernels and the `_dyn` pixel kernels instead of one launch per class.
    uint32_t *d_stats = nullptr;        // RS_WORDS per image
    uint8_t *d_host_cls = nullptr;      // per image * 4 + comp: 0 / 1 / 3 or CLS_FROM_DEVICE
    static constexpr int kClsRing = 4;
    uint8_t *h_host_cls = nullptr;      // pinned, kClsRing copies (the upload is asynchronous on the decode stream)
    hipEvent_t cls_sent[kClsRing] = {nullptr, nullptr, nullptr, nullptr};
    uint32_t cls_next = 0;
    uint32_t *d_plane_job_slot = nullptr;  // generic path: plane job -> image * 4 + comp
    std::vector<uint8_t> cls_src;
    bool dev_classes = false;
    bool cls_dirty = true;              // class knowledge changed since the tables / the class table were last sent
    // JPGPU_BATCH_KERNEL_TIMES (diagnostics, jpgpu_pipeline_timings): events around the phases of the device entropy path
    hipEvent_t ev_phase[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool phase_events_valid = false;
    bool progressive_launch = false;  // the last device entropy launch was batch_device_progressive_launch
    // Entry-list pixel path (fused_entries.hpp): images whose last device entropy launch kept their scan as entry lists.  entry_img[image]
    // = 1 until the host uploads coefficients for the image (a re-decode): the dense kernels skip it (CLS_SKIP), the decode that follows
    // the launch on its stream runs s420_entries_kernel over the plan(s) and copies the status words once more behind it.
    // Every writer that makes the coefficient arena an image's source again drops the flag: per image, batch_drop_entry_image (host
    // uploads dense or compact, classes set from the host); for the whole batch, batch_drop_entries (the device entropy and progressive
    // launches, jpgpu_batch_classify_on_device).  A flag left behind has the next decode skip the image and return its old pixels.
    std::vector<uint8_t> entry_img;
    bool entries_pending = false;
    const EntrySrc *d_entry_srcs = nullptr;   // per batch image, inside d_entropy
    const uint32_t *d_entry_status = nullptr; // the launch's status words (device) and how many
    uint32_t entry_status_n = 0;
};

#define B_HIP(call)                                                                                     \
    do {                                                                                                \
        hipError_t _e = (call);                                                                         \
        if (_e != hipSuccess) return set_err(b->err, JPGPU_ERR_IO, "%s: %s", #call, hipGetErrorString(_e)); \
    } while (0)

// before a blocking rewrite of anything enqueued work reads (see jpgpu_batch::enqueued); free when nothing was enqueued since the last wait
static hipError_t batch_wait_enqueued(jpgpu_batch *b) {
    if (!b->enqueue_pending) return hipSuccess;
    b->enqueue_pending = false;
    return hipEventSynchronize(b->enqueued);
}
static hipError_t batch_mark_enqueued(jpgpu_batch *b, hipStream_t s) {
    const hipError_t e = hipEventRecord(b->enqueued, s);
    if (e == hipSuccess) b->enqueue_pending = true;
    return e;
}

// where the pixel kernels write: the output arena, or the intermediate one of a batch with an output size
static uint8_t *pix_base(const jpgpu_batch *b) { return b->o.spec.w ? b->o.d_pix : b->d_out; }
static const std::vector<size_t> &pix_offsets(const jpgpu_batch *b) { return b->o.spec.w ? b->o.pix_off : b->out_off; }

// first use of the device-side classes: statistics (zeroed), class table, pinned staging
static int batch_enable_dev_classes(jpgpu_batch *b) {
    if (b->d_stats) return JPGPU_OK;
    const size_t n = b->descs.size();
    B_HIP(hipMalloc((void **)&b->d_stats, n * RS_WORDS * sizeof(uint32_t)));
    B_HIP(hipMemset(b->d_stats, 0, n * RS_WORDS * sizeof(uint32_t)));
    B_HIP(hipMalloc((void **)&b->d_host_cls, n * 4));
    B_HIP(hipHostMalloc((void **)&b->h_host_cls, n * 4 * jpgpu_batch::kClsRing, hipHostMallocDefault));
    for (auto &e : b->cls_sent) B_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (!b->generic_ids.empty()) B_HIP(hipMalloc((void **)&b->d_plane_job_slot, n * 4 * sizeof(uint32_t)));
    b->jobs_dirty = true;  // (the plane-job slot table goes up with the jobs)
    return JPGPU_OK;
}

// mark component `idx` = image * 4 + comp as classified by the device statistics / by the host (`sane[idx]`)
static void batch_class_source(jpgpu_batch *b, size_t idx, bool from_device) {
    if (b->cls_src[idx] != (from_device ? 1 : 0)) {
        b->cls_src[idx] = from_device ? 1 : 0;
        b->cls_dirty = true;
    }
    if (from_device) b->dev_classes = true;
}
// the image's pixels come from the coefficient arena again (see entry_img)
static void batch_drop_entry_image(jpgpu_batch *b, size_t image) {
    if (image < b->entry_img.size() && b->entry_img[image]) {
        b->entry_img[image] = 0;
        b->cls_dirty = true;
    }
}
// the same for every image, and no entry-list walk owed to an earlier launch
static void batch_drop_entries(jpgpu_batch *b) {
    if (b->entry_img.size() != b->descs.size()) b->entry_img.assign(b->descs.size(), 0);
    for (size_t i = 0; i < b->entry_img.size(); i++) batch_drop_entry_image(b, i);
    b->entries_pending = false;
}
static void batch_set_host_class(jpgpu_batch *b, size_t idx, uint8_t cls) {
    batch_drop_entry_image(b, idx / 4);  // coefficients from the host: the image is a dense one again
    if (b->sane[idx] != cls) {
        b->sane[idx] = cls;
        b->cls_dirty = true;
    }
    batch_class_source(b, idx, false);
}

// the status words of a launch into b->h_entropy_out (pinned), behind the kernels on `s`: by a kernel, not by the copy engine (huff.hip)
static hipError_t batch_status_to_host(jpgpu_batch *b, const uint32_t *d_status, uint32_t n, hipStream_t s) {
    void *mapped = nullptr;
    hipError_t e = hipHostGetDevicePointer(&mapped, b->h_entropy_out, 0);
    if (e != hipSuccess) {  // (no mapping: the copy engine after all)
        (void)hipGetLastError();
        return hipMemcpyAsync(b->h_entropy_out, d_status, (size_t)n * 4, hipMemcpyDeviceToHost, s);
    }
    return launch_copy_words_to_host(static_cast<uint32_t *>(mapped), d_status, n, s);
}
static uint32_t env_u32(const char *name, uint32_t dflt, uint32_t lo, uint32_t hi) {
    const char *e = getenv(name);
    if (!e || !*e) return dflt;
    const long v = atol(e);
    return (uint32_t)std::min<long>(std::max<long>(v, lo), hi);
}

// component `c` of image `i` as a PlaneJob: where its coefficients and its table lie (the generic path adds its plane and class)
static PlaneJob batch_plane_job(const jpgpu_batch *b, uint32_t i, uint32_t c) {
    const jpgpu_component &cc = b->descs[i].components[c];
    PlaneJob j{};
    j.coefs = reinterpret_cast<const int16_t *>(b->d_coef + b->coef_off[i * 4 + c]);
    j.qt = b->d_qt + ((size_t)i * 4 + c) * 64;
    j.block_w = cc.block_width;
    j.n_blocks = (uint32_t)cc.block_width * cc.block_height;
    j.scale = cc.dct_scale;
    return j;
}
template <typename Geom>
int BandGroup<Geom>::fill_jobs(jpgpu_batch *b, uint8_t *pix, const std::vector<size_t> &pix_off) {
    plane_jobs.clear();
    image_jobs.clear();
    for (uint32_t i : ids) {  // (the reduced IDCTs and the window kernel are exact at any class; job.out = the image's or the window's bytes)
        const jpgpu_image_desc &d = b->descs[i];
        uint8_t *no_planes[4] = {nullptr, nullptr, nullptr, nullptr};
        for (uint32_t c = 0; c < d.ncomp; c++) plane_jobs.push_back(batch_plane_job(b, i, c));
        ImageJob ij;
        size_t out_len = 0;
        int rc = build_image_job(d.components, d.ncomp, no_planes, d.out_w, d.out_h, d.color_transform, pix + pix_off[i], ij, out_len, b->err);
        if (rc) return rc;
        image_jobs.push_back(ij);
    }
    if (!plane_jobs.empty()) {  // (batch_refresh_jobs has waited for the decodes enqueued: batch_wait_enqueued)
        B_HIP(hipMemcpy(d_plane_jobs, plane_jobs.data(), plane_jobs.size() * sizeof(PlaneJob), hipMemcpyHostToDevice));
        B_HIP(hipMemcpy(d_image_jobs, image_jobs.data(), image_jobs.size() * sizeof(ImageJob), hipMemcpyHostToDevice));
    }
    return JPGPU_OK;
}

// Buffers that grow on demand (the caller has found `need` above `cap`): free, allocate `want` elements — a quarter more than needed
// unless the caller says otherwise —, and the capacity stands only once the block does.  (hipFree waits for whatever still uses the block.)
template <typename T>
static hipError_t grow_device(T *&p, size_t &cap, size_t need, size_t want = 0) {
    if (p) (void)hipFree(p);
    p = nullptr, cap = 0;
    if (!want) want = quarter_more(need);
    const hipError_t e = hipMalloc((void **)&p, want * sizeof(T));
    if (e == hipSuccess) cap = want;
    return e;
}
template <typename T>
static hipError_t grow_pinned(T *&p, size_t &cap, size_t need, size_t want = 0) {
    if (p) (void)hipHostFree(p);
    p = nullptr, cap = 0;
    if (!want) want = quarter_more(need);
    const hipError_t e = hipHostMalloc((void **)&p, want * sizeof(T), hipHostMallocDefault);
    if (e == hipSuccess) cap = want;
    return e;
}
