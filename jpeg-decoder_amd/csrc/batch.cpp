// batch.cpp — batch driver of the C ABI (include/jpgpu.h, jpgpu_batch_*).
//
// A batch is N independent images (the unit the reference decodes one-per-Decoder,
// src/decoder.rs:134-154) laid out in two HBM arenas: all coefficient planes (int16,
// block-raster = the concatenation of each component's append_row buffers)
// and all output pixels.  One decode = a handful of launches over the whole batch.
// Images of a fusable kind (4:2:0 YCbCr, 4:4:4 YCbCr / RGB, gray; any size) are grouped per kind and run the fused
// kernels (fused.hip), one launch group per kind; everything else runs the generic two-kernel path (kernels.hip)
// through device job tables.  jpgpu_batch_path names the kernels: "fused420", ..., "generic", or "mixed".
#include <array>
#include <map>

#include "batch_internal.hpp"

// The resample tables and bands of every image from its source size (its window's, else its output grid's): at creation and after
// batch_rewindow.  Axes of equal (in, out) sizes share one table.
static int batch_resample_tables(jpgpu_batch *b) {
    const uint32_t n = (uint32_t)b->descs.size();
    b->rs_jobs.assign(n, ResampleJob{});
    b->rs_tab.clear();
    b->rs_max_bands = b->rs_lds_bytes = b->rs_max_runs = 0;
    b->rs_bpr.assign(n, 0u);
    std::map<uint64_t, std::pair<uint32_t, uint32_t>> seen;  // (in, out) -> offsets of bounds, coefficients
    const uint32_t filter = b->filter;                       // (one per batch: the keys need not hold it)
    auto axis = [&](uint32_t in, uint32_t out, uint32_t &bo, uint32_t &ko, uint32_t &ks) {
        ks = resample_ksize_filtered(filter, in, out);
        const uint64_t key = ((uint64_t)in << 32) | out;
        auto it = seen.find(key);
        if (it != seen.end()) return bo = it->second.first, ko = it->second.second, true;
        const size_t base = b->rs_tab.size(), end = base + 2u * (size_t)out + (size_t)out * ks;
        if (end > 0xffffffffull) return false;
        b->rs_tab.resize(end);
        bo = (uint32_t)base, ko = (uint32_t)(base + 2u * out);
        resample_coefficients_filtered(filter, in, out, b->rs_tab.data() + bo, b->rs_tab.data() + ko, ks);
        seen[key] = {bo, ko};
        return true;
    };
    // a placed batch: entries [first, first + count) of the axis (in, out) — the visible range, nothing else is tabulated
    std::map<std::array<uint32_t, 4>, std::pair<uint32_t, uint32_t>> seen_range;
    auto axis_range = [&](uint32_t in, uint32_t out, uint32_t first, uint32_t count, uint32_t &bo, uint32_t &ko, uint32_t &ks) {
        ks = resample_ksize_filtered(filter, in, out);
        const std::array<uint32_t, 4> key = {in, out, first, count};
        auto it = seen_range.find(key);
        if (it != seen_range.end()) return bo = it->second.first, ko = it->second.second, true;
        const size_t base = b->rs_tab.size(), end = base + 2u * (size_t)count + (size_t)count * ks;
        if (end > 0xffffffffull) return false;
        b->rs_tab.resize(end);
        bo = (uint32_t)base, ko = (uint32_t)(base + 2u * count);
        resample_coefficients_range_filtered(filter, in, out, first, count, b->rs_tab.data() + bo, b->rs_tab.data() + ko, ks);
        seen_range[key] = {bo, ko};
        return true;
    };
    if (b->placed) b->rs_places.assign(n, Place{});
    size_t k = 0;
    for (uint32_t i = 0; i < n; i++) {
        const jpgpu_image_desc &d = b->descs[i];
        ResampleJob &j = b->rs_jobs[i];
        window_grid(d.components, d.ncomp, d.out_w, d.out_h, j.in_w, j.in_h);
        if (k < b->win.ids.size() && b->win.ids[k] == i) j.in_w = b->win.geoms[k].ww, j.in_h = b->win.geoms[k].wh, k++;
        j.nc = d.ncomp, j.out_w = b->rs_w, j.out_h = b->rs_h;
        if (b->flags & JPGPU_BATCH_RGB_OUTPUT) j.nc = 3u, j.src_nc = d.ncomp == 3u ? 0u : d.ncomp;  // (gray / CMYK: converted by the horizontal pass)
        if (b->placed) {  // (the job of the visible rectangle)
            const jpgpu_placement &pl = b->pl[i];
            Place &p = b->rs_places[i];
            uint32_t fx = 0, fy = 0;
            if (!placed_axis(pl.rw, pl.x, b->rs_w, fx, j.out_w, p.vx) || !placed_axis(pl.rh, pl.y, b->rs_h, fy, j.out_h, p.vy))
                return set_err(b->err, JPGPU_ERR_FORMAT, "image %u: the placement shows no pixel", i);
            p.cw = b->rs_w, p.ch = b->rs_h, p.fill = b->pl_fill;
            if (!axis_range(j.in_w, pl.rw, fx, j.out_w, j.hb, j.hk, j.hks) || !axis_range(j.in_h, pl.rh, fy, j.out_h, j.vb, j.vk, j.vks))
                return set_err(b->err, JPGPU_ERR_UNSUPPORTED, "image %u: resample tables of the batch exceed 2^32 words", i);
            continue;
        }
        if (!axis(j.in_w, j.out_w, j.hb, j.hk, j.hks) || !axis(j.in_h, j.out_h, j.vb, j.vk, j.vks))
            return set_err(b->err, JPGPU_ERR_UNSUPPORTED, "image %u: resample tables of the batch exceed 2^32 words", i);
    }
    for (uint32_t i = 0; i < n; i++) {  // (the tables stand still now)
        ResampleJob &j = b->rs_jobs[i];
        if (b->placed) {
            if (!placed_plan(j, b->rs_places[i], b->rs_tab.data())) return set_err(b->err, JPGPU_ERR_INTERNAL, "image %u: no resample plan", i);
            b->rs_max_bands = std::max(b->rs_max_bands, b->rs_places[i].bands);
        } else {
            if (!resample_plan(j, b->rs_tab.data())) return set_err(b->err, JPGPU_ERR_INTERNAL, "image %u: no resample plan", i);
            // (JPGPU_RS_ROLL, read per call: 1 never, 2 / 4 / 8 every candidate with that many bands per run — the benchmark's A/B)
            const char *knob = getenv("JPGPU_RS_ROLL");
            const uint32_t bpr = b->rs_bpr[i] = resample_roll_bpr(j, b->rs_tab.data(), filter, knob ? (uint32_t)atoi(knob) : 0u);
            if (bpr) b->rs_max_runs = std::max(b->rs_max_runs, (j.bands + bpr - 1u) / bpr);
            else b->rs_max_bands = std::max(b->rs_max_bands, j.bands);
        }
        b->rs_lds_bytes = std::max(b->rs_lds_bytes, j.lds_bytes);
    }
    const size_t roll_at = b->path.find("+roll");  // (the path names the route where any image took it; other windows may change that)
    if (roll_at != std::string::npos) b->path.erase(roll_at, 5);
    if (b->rs_max_runs) b->path.insert(std::min(b->path.find("+warp"), b->path.size()), "+roll");  // (the last word of the u8 batch's path: in front of a warp's)
    B_HIP(batch_wait_enqueued(b));  // (a decode still queued reads the tables)
    if (b->rs_tab.size() > b->rs_tab_cap) {
        B_HIP(hipDeviceSynchronize());
        B_HIP(grow_device(b->d_rs_tab, b->rs_tab_cap, b->rs_tab.size()));
    }
    B_HIP(hipMemcpy(b->d_rs_tab, b->rs_tab.data(), b->rs_tab.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (b->d_rs_bpr) B_HIP(hipMemcpy(b->d_rs_bpr, b->rs_bpr.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    b->jobs_dirty = true;  // (the jobs go up with the others)
    return JPGPU_OK;
}

// every image's quantization tables to the device (unused slots: ones)
static int batch_upload_qt(jpgpu_batch *b) {
    const uint32_t n = (uint32_t)b->descs.size();
    std::vector<uint16_t> qt((size_t)n * 4 * 64, 1);
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t c = 0; c < b->descs[i].ncomp; c++)
            memcpy(&qt[((size_t)i * 4 + c) * 64], b->descs[i].quantization_tables[c], 128);
    B_HIP(hipMemcpy(b->d_qt, qt.data(), qt.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    return JPGPU_OK;
}

// The TensorJobs of a tensor batch: every image's resample job, its plane pitch and its flip.  They travel on the decode's stream from a
// pinned mirror (fresh flips come with every call of a loader: a blocking copy per sub-batch would hold the uploader thread up).
static int batch_upload_tensor_jobs(jpgpu_batch *b, hipStream_t stream) {
    const uint32_t n = (uint32_t)b->descs.size();
    if (!b->h_tn_jobs && !b->h_ptn_jobs) {
        if (b->placed) B_HIP(hipHostMalloc((void **)&b->h_ptn_jobs, (size_t)n * sizeof(PlacedTensorJob), hipHostMallocDefault));
        else B_HIP(hipHostMalloc((void **)&b->h_tn_jobs, (size_t)n * 2u * sizeof(TensorJob), hipHostMallocDefault));
        B_HIP(hipEventCreateWithFlags(&b->tn_sent, hipEventDisableTiming));
    } else {
        B_HIP(hipEventSynchronize(b->tn_sent));  // (the copy before this one has read the mirror)
    }
    if (b->placed) {  // (the same records with every image's placement behind them)
        for (uint32_t i = 0; i < n; i++) {
            b->h_ptn_jobs[i].t.r = b->rs_jobs[i];
            b->h_ptn_jobs[i].t.plane = b->rs_w * b->rs_h;
            b->h_ptn_jobs[i].t.flip = b->tn_flips[i] ? 1u : 0u;
            b->h_ptn_jobs[i].p = b->rs_places[i];
        }
        B_HIP(hipMemcpyAsync(b->d_ptn_jobs, b->h_ptn_jobs, (size_t)n * sizeof(PlacedTensorJob), hipMemcpyHostToDevice, stream));
        B_HIP(hipEventRecord(b->tn_sent, stream));
        b->tn_dirty = false;
        return JPGPU_OK;
    }
    for (uint32_t i = 0; i < n; i++) {
        b->h_tn_jobs[i].r = b->rs_jobs[i];
        b->h_tn_jobs[i].plane = b->rs_w * b->rs_h;
        b->h_tn_jobs[i].flip = b->tn_flips[i] ? 1u : 0u;
        if (!b->rs_max_runs) continue;
        b->h_tn_jobs[n + i] = b->h_tn_jobs[i];               // (the run launch's: the real job)
        if (b->rs_bpr[i]) b->h_tn_jobs[i].r.bands = 0u;  // (the band launch's: no band of this image)
    }
    B_HIP(hipMemcpyAsync(b->d_tn_jobs, b->h_tn_jobs, (size_t)n * (b->rs_max_runs ? 2u : 1u) * sizeof(TensorJob), hipMemcpyHostToDevice, stream));
    B_HIP(hipEventRecord(b->tn_sent, stream));
    b->tn_dirty = false;
    return JPGPU_OK;
}

// The WarpJobs of a warped batch and the N-sep tables behind them: every image's matrix, its flip, where it reads and writes.  From a
// pinned mirror on the decode's stream, as the TensorJobs: a decode queued earlier keeps the matrices it was enqueued with.
static size_t warp_jobs_bytes(const jpgpu_batch *b) { return b->descs.size() * (sizeof(WarpJob) + ((size_t)b->rs_w + b->rs_h) * sizeof(int32_t)); }
static int batch_upload_warp_jobs(jpgpu_batch *b, hipStream_t stream) {
    const uint32_t n = (uint32_t)b->descs.size();
    if (!b->h_wp_jobs) {
        B_HIP(hipHostMalloc((void **)&b->h_wp_jobs, warp_jobs_bytes(b), hipHostMallocDefault));
        B_HIP(hipEventCreateWithFlags(&b->wp_sent, hipEventDisableTiming));
    } else {
        B_HIP(hipEventSynchronize(b->wp_sent));  // (the copy before this one has read the mirror)
    }
    WarpJob *jobs = reinterpret_cast<WarpJob *>(b->h_wp_jobs);
    int32_t *tabs = reinterpret_cast<int32_t *>(b->h_wp_jobs + (size_t)n * sizeof(WarpJob));
    const bool rgb = (b->flags & JPGPU_BATCH_RGB_OUTPUT) != 0;
    for (uint32_t i = 0; i < n; i++) {
        WarpJob &j = jobs[i];
        j.src = b->d_wsrc + b->wsrc_off[i], j.dst = b->d_out + b->out_off[i];
        j.w = b->rs_w, j.h = b->rs_h, j.nc = rgb ? 3u : b->descs[i].ncomp;
        j.flip = (b->tn_es && b->tn_flips[i]) ? 1u : 0u;
        j.fill = b->wp_fill, j.plane = b->rs_w * b->rs_h;
        j.tab = i * (b->rs_w + b->rs_h);
        warp_job_matrix(j, b->wp_m[i].m, b->wp_filter, tabs + j.tab);
    }
    B_HIP(hipMemcpyAsync(b->d_wp_jobs, b->h_wp_jobs, warp_jobs_bytes(b), hipMemcpyHostToDevice, stream));
    B_HIP(hipEventRecord(b->wp_sent, stream));
    b->wp_dirty = false;
    return JPGPU_OK;
}

static int batch_refresh_jobs(jpgpu_batch *b, hipStream_t stream = nullptr) {
    // host-side classes are part of the launch tables (one launch per class: fused_bind); with device-side classes they
    // travel in a small table of their own, asynchronously, and the launch tables stay as they are
    const bool need_bind = b->jobs_dirty || (b->cls_dirty && !b->dev_classes);
    if (!need_bind && b->tn_dirty && b->d_coef && b->d_out) {  // (other flips alone: the TensorJobs, nothing else)
        int rc = batch_upload_tensor_jobs(b, stream);
        if (rc) return rc;
    }
    if (!need_bind && b->wp_dirty && b->d_coef && b->d_out) {  // (other matrices or flips alone: the WarpJobs, nothing else)
        int rc = batch_upload_warp_jobs(b, stream);
        if (rc) return rc;
    }
    if (!need_bind && !b->cls_dirty) return JPGPU_OK;
    if (!b->d_coef || !b->d_out) return set_err(b->err, JPGPU_ERR_FORMAT, "batch has no device buffers bound");
    // The tables below go up by blocking copies on the null stream, which nothing orders behind a decode still queued on a non-blocking
    // stream: that decode would read the next one's tables.  (The class table and the TensorJobs travel on `stream` itself.)
    if (need_bind) B_HIP(batch_wait_enqueued(b));
    uint8_t *const pix = pix_base(b);
    const std::vector<size_t> &pix_off = pix_offsets(b);
    if (b->dev_classes) {
        const size_t n4 = b->descs.size() * 4;
        const uint32_t k = b->cls_next++ % jpgpu_batch::kClsRing;
        uint8_t *h = b->h_host_cls + (size_t)k * n4;
        B_HIP(hipEventSynchronize(b->cls_sent[k]));  // (its previous copy, four refreshes ago: long gone)
        for (size_t i = 0; i < n4; i++) h[i] = (i / 4 < b->entry_img.size() && b->entry_img[i / 4]) ? CLS_SKIP : (b->cls_src[i] ? CLS_FROM_DEVICE : b->sane[i]);
        B_HIP(hipMemcpyAsync(b->d_host_cls, h, n4, hipMemcpyHostToDevice, stream));
        B_HIP(hipEventRecord(b->cls_sent[k], stream));
    }
    b->cls_dirty = false;
    if (!need_bind) return JPGPU_OK;
    const uint32_t n = (uint32_t)b->descs.size();
    b->plane_jobs.clear();
    b->image_jobs.clear();
    for (uint32_t i : b->generic_ids) {
        const jpgpu_image_desc &d = b->descs[i];
        uint8_t *planes[4] = {nullptr, nullptr, nullptr, nullptr};
        for (uint32_t c = 0; c < d.ncomp; c++) {
            PlaneJob j = batch_plane_job(b, i, c);
            j.plane = b->d_planes ? b->d_planes + b->plane_off[i * 4 + c] : nullptr;
            j.flags = b->sane[i * 4 + c];
            planes[c] = j.plane;
            b->plane_jobs.push_back(j);
        }
        ImageJob ij;
        size_t out_len = 0;
        int rc = build_image_job(d.components, d.ncomp, planes, d.out_w, d.out_h, d.color_transform,
                                 pix + pix_off[i], ij, out_len, b->err);
        if (rc) return rc;
        b->image_jobs.push_back(ij);
    }
    if (!b->plane_jobs.empty())
        B_HIP(hipMemcpy(b->d_plane_jobs, b->plane_jobs.data(), b->plane_jobs.size() * sizeof(PlaneJob), hipMemcpyHostToDevice));
    if (!b->plane_jobs.empty() && b->d_plane_job_slot) {
        std::vector<uint32_t> slots;
        for (uint32_t i : b->generic_ids)
            for (uint32_t c = 0; c < b->descs[i].ncomp; c++) slots.push_back(i * 4 + c);
        B_HIP(hipMemcpy(b->d_plane_job_slot, slots.data(), slots.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (!b->image_jobs.empty())
        B_HIP(hipMemcpy(b->d_image_jobs, b->image_jobs.data(), b->image_jobs.size() * sizeof(ImageJob), hipMemcpyHostToDevice));
    int rc = b->scaled.fill_jobs(b, pix, pix_off);
    if (rc == JPGPU_OK) rc = b->win.fill_jobs(b, pix, pix_off);
    if (rc) return rc;
    for (FusedPlan &fp : b->fused) {
        rc = fused_bind(fp, b->d_coef, pix, b->d_qt, b->coef_off, pix_off, b->sane, b->err);
        if (rc) return rc;
    }
    if (b->rs_w) {
        for (uint32_t i = 0; i < n; i++) b->rs_jobs[i].src = pix + pix_off[i], b->rs_jobs[i].dst = b->warp ? b->d_wsrc + b->wsrc_off[i] : b->d_out + b->out_off[i];
        if (b->warp) {  // (the u8 resample of the same arguments writes the warp's source; the warp writes the output)
            rc = batch_upload_warp_jobs(b, stream);
            if (rc) return rc;
        }
        if (b->tn_es && !b->warp) {
            rc = batch_upload_tensor_jobs(b, stream);
            if (rc) return rc;
        } else if (b->placed) {
            std::vector<PlacedJob> pj(n);
            for (uint32_t i = 0; i < n; i++) pj[i].r = b->rs_jobs[i], pj[i].p = b->rs_places[i];
            B_HIP(hipMemcpy(b->d_pl_jobs, pj.data(), (size_t)n * sizeof(PlacedJob), hipMemcpyHostToDevice));
        } else if (b->rs_max_runs) {  // (band launch: images in runs have no band; run launch: the real jobs)
            std::vector<ResampleJob> both(b->rs_jobs);
            both.insert(both.end(), b->rs_jobs.begin(), b->rs_jobs.end());
            for (uint32_t i = 0; i < n; i++)
                if (b->rs_bpr[i]) both[i].bands = 0u;
            B_HIP(hipMemcpy(b->d_rs_jobs, both.data(), (size_t)n * 2u * sizeof(ResampleJob), hipMemcpyHostToDevice));
        } else {
            B_HIP(hipMemcpy(b->d_rs_jobs, b->rs_jobs.data(), (size_t)n * sizeof(ResampleJob), hipMemcpyHostToDevice));
        }
    }
    if (b->qt_dirty) {
        rc = batch_upload_qt(b);
        if (rc) return rc;
        b->qt_dirty = false;
    }
    b->jobs_dirty = false;
    return JPGPU_OK;
}

extern "C" {

// rs_w, rs_h: the output size of jpgpu_batch_create_resized (0, 0: none); tensor: the format of jpgpu_batch_create_tensor (NULL: none)
// placements, fill: those of jpgpu_batch_create_placed (NULL: none)
static int batch_create(int device, const jpgpu_image_desc *descs, const jpgpu_window *windows, uint32_t rs_w, uint32_t rs_h,
                        const jpgpu_tensor_format *tensor, uint32_t n_images, uint32_t flags, jpgpu_batch **out,
                        const jpgpu_placement *placements = nullptr, const uint8_t *fill = nullptr, const jpgpu_warp_options *warp = nullptr) {
    if (!out) return JPGPU_ERR_FORMAT;
    *out = nullptr;
    if (!descs || n_images == 0 || n_images > 65535) return JPGPU_ERR_FORMAT;
    jpgpu_batch *b = new jpgpu_batch();
    *out = b;  // returned even on failure so the caller can read last_error, then destroy
    b->device = device;
    b->flags = flags;
    const bool resized = rs_w != 0 || rs_h != 0;
    if (resized && (rs_w == 0 || rs_h == 0 || rs_w > RS_MAX_OUT || rs_h > RS_MAX_OUT))
        return set_err(b->err, JPGPU_ERR_FORMAT, "output size %ux%u: width and height must be 1..%u", rs_w, rs_h, RS_MAX_OUT);
    const uint32_t filter = (flags >> 8) & 15u;  // JPGPU_BATCH_FILTER(f): 0 is BILINEAR, so flags without the bits mean what they meant
    if (filter >= RS_FILTERS) return set_err(b->err, JPGPU_ERR_FORMAT, "resample filter %u: the ids are 0..%u (JPGPU_FILTER_*)", filter, RS_FILTERS - 1u);
    if (filter && !resized)
        return set_err(b->err, JPGPU_ERR_UNSUPPORTED, "a resample filter (%s) needs an output size (jpgpu_batch_create_resized / _create_tensor / _create_placed)",
                       resample_filter_name(filter));
    b->filter = filter;
    const bool rgb = (flags & JPGPU_BATCH_RGB_OUTPUT) != 0;  // (every image gives three channels: the resample converts gray and CMYK)
    if (rgb && !resized)
        return set_err(b->err, JPGPU_ERR_UNSUPPORTED, "JPGPU_BATCH_RGB_OUTPUT needs an output size (jpgpu_batch_create_resized / _create_tensor)");
    if (warp) {  // (every image starts with the identity)
        if (!resized) return set_err(b->err, JPGPU_ERR_FORMAT, "a warp needs an output size");
        if (warp->filter > WP_BILINEAR || warp->reserved != 0)
            return set_err(b->err, JPGPU_ERR_FORMAT, "warp options: filter %u, reserved %u (JPGPU_WARP_NEAREST or JPGPU_WARP_BILINEAR, reserved 0)", warp->filter, warp->reserved);
        b->warp = true, b->wp_filter = warp->filter;
        b->wp_fill = (uint32_t)warp->fill[0] | ((uint32_t)warp->fill[1] << 8) | ((uint32_t)warp->fill[2] << 16) | ((uint32_t)warp->fill[3] << 24);
        b->wp_m.assign(n_images, jpgpu_warp{{1.0, 0.0, 0.0, 0.0, 1.0, 0.0}});
    }
    if (tensor) {  // (the format against the channels of every image of the call, before anything is allocated)
        if (!resized) return set_err(b->err, JPGPU_ERR_FORMAT, "a tensor format needs an output size");
        uint32_t nc_max = rgb ? 3u : 1u;
        for (uint32_t i = 0; i < n_images && !rgb; i++) nc_max = std::max(nc_max, std::min<uint32_t>(descs[i].ncomp, 4u));
        const char *why = nullptr;
        if (!tensor_format_ok(tensor->dtype, tensor->reserved, tensor->mean, tensor->std, nc_max, why)) return set_err(b->err, JPGPU_ERR_FORMAT, "tensor format: %s", why);
    }
    if (placements && resized) {  // (every placement shows a pixel; one that differs from the whole output makes the batch a placed one)
        b->pl.assign(placements, placements + n_images);
        for (uint32_t i = 0; i < n_images; i++) {
            jpgpu_placement &pl = b->pl[i];
            if (pl.rw == 0 || pl.rh == 0) pl = jpgpu_placement{(uint16_t)rs_w, (uint16_t)rs_h, 0, 0};
            uint32_t first, count, v0;
            if (!placed_axis(pl.rw, pl.x, rs_w, first, count, v0) || !placed_axis(pl.rh, pl.y, rs_h, first, count, v0))
                return set_err(b->err, JPGPU_ERR_FORMAT, "image %u: the placement %ux%u at (%d, %d) shows no pixel of the %ux%u output", i, pl.rw, pl.rh, pl.x, pl.y,
                               rs_w, rs_h);
            if (pl.rw != rs_w || pl.rh != rs_h || pl.x != 0 || pl.y != 0) b->placed = true;
        }
        if (fill) b->pl_fill = (uint32_t)fill[0] | ((uint32_t)fill[1] << 8) | ((uint32_t)fill[2] << 16) | ((uint32_t)fill[3] << 24);
    }
    int rc = use_device(device, b->err);
    if (rc) return rc;
    b->descs.assign(descs, descs + n_images);
    b->coef_off.assign((size_t)n_images * 4, 0);
    b->coef_len.assign((size_t)n_images * 4, 0);
    b->plane_off.assign((size_t)n_images * 4, 0);
    b->out_full_len.assign(n_images, 0);
    b->sane.assign((size_t)n_images * 4, 0);
    b->cls_src.assign((size_t)n_images * 4, 0);
    // path resolution: group the images that can share a fused launch, the rest is generic
    std::vector<uint32_t> kind_key(n_images, 0);
    if (!(flags & JPGPU_BATCH_FORCE_GENERIC))
        for (uint32_t i = 0; i < n_images; i++)
            if (b->descs[i].ncomp >= 1 && b->descs[i].ncomp <= 4) kind_key[i] = fused_kind_key(b->descs[i]);
    size_t co = 0, po = 0;
    std::vector<size_t> lens(n_images, 0);  // per image: bytes of what its pixel kernel writes
    for (uint32_t i = 0; i < n_images; i++) {
        const jpgpu_image_desc &d = b->descs[i];
        if (d.ncomp == 0 || d.ncomp > 4) return set_err(b->err, JPGPU_ERR_FORMAT, "image %u: bad component count %u", i, d.ncomp);
        // validate once with dummy plane pointers (same checks as compute_image)
        uint8_t *dummy[4] = {nullptr, nullptr, nullptr, nullptr};
        ImageJob ij;
        size_t out_len = 0;
        rc = build_image_job(d.components, d.ncomp, dummy, d.out_w, d.out_h, d.color_transform, nullptr, ij, out_len, b->err);
        if (rc) return rc;
        b->out_full_len[i] = out_len;
        if (resized && ij.color_fn == CC_NONE && d.ncomp > 1)
            return set_err(b->err, JPGPU_ERR_UNSUPPORTED, "image %u: no output size for planar output (ColorTransform None with %u components)", i, d.ncomp);
        if (rgb && d.ncomp != 1 && d.ncomp != 3 && d.ncomp != 4) return set_err(b->err, JPGPU_ERR_UNSUPPORTED, "image %u: no RGB output for %u components", i, d.ncomp);
        // a window smaller than the image: the window group (an empty window or one that covers the image is no window)
        bool windowed = false;
        if (windows) {
            uint32_t gw = 0, gh = 0;
            WindowGeom wg;
            std::string why;
            rc = window_rule(d, windows[i], windowed, gw, gh, wg, why);
            if (rc) return set_err(b->err, rc, "image %u: %s", i, why.c_str());
            if (windowed) {
                kind_key[i] = 0;
                b->win.add(i, wg);
                out_len = (size_t)wg.ww * wg.wh * d.ncomp;
            }
        }
        // reduced-size decodes (every component at one dct_scale < 8): one launch, planes in LDS (fused_scaled.hpp)
        ScaledGeom sg;
        static const uint32_t scaled_tx = getenv("JPGPU_SCALED_TX") ? (uint32_t)std::max(8, atoi(getenv("JPGPU_SCALED_TX"))) : 64u;  // (tuning / test knob)
        static const uint32_t scaled_ry = getenv("JPGPU_SCALED_RY") ? (uint32_t)std::max(1, atoi(getenv("JPGPU_SCALED_RY"))) : 8u;
        const bool scaled = !windowed && kind_key[i] == 0 && !(flags & JPGPU_BATCH_FORCE_GENERIC) && scaled_geom_from_job(d.components, d.ncomp, ij, sg, scaled_tx, scaled_ry);
        if (scaled) {
            b->scaled.add(i, sg);
            const char *nm = scaled_path_name(sg);
            if (b->scaled_name.empty()) b->scaled_name = nm;
            else if (b->scaled_name != nm) b->scaled_name = "fusedscaled-mixed";
        }
        for (uint32_t c = 0; c < d.ncomp; c++) {
            const jpgpu_component &cc = d.components[c];
            size_t cb = (size_t)cc.block_width * cc.block_height * 64 * sizeof(int16_t);
            b->coef_off[i * 4 + c] = co;
            b->coef_len[i * 4 + c] = cb;
            co += align_up(cb, 256);
            if (kind_key[i] == 0 && !scaled && !windowed) {  // generic path: intermediate u8 plane, launch extents
                b->plane_off[i * 4 + c] = po;
                po += align_up(plane_bytes(cc), 256);
                b->max_blocks = std::max<uint32_t>(b->max_blocks, (uint32_t)cc.block_width * cc.block_height);
                b->scales[cc.dct_scale] = true;
            }
        }
        lens[i] = out_len;
        if (kind_key[i] == 0 && !scaled && !windowed) {
            b->generic_ids.push_back(i);
            b->max_w = std::max<uint32_t>(b->max_w, d.ncomp == 1 ? d.components[0].size_width : d.out_w);
            b->max_h = std::max<uint32_t>(b->max_h, d.ncomp == 1 ? d.components[0].size_height : d.out_h);
        }
    }
    b->coef_bytes = std::max<size_t>(co, 256);
    b->out_bytes = arena_layout(lens, b->out_off, b->out_len);
    b->plane_bytes_total = std::max<size_t>(po, 256);
    if (resized) {  // what was laid out so far is the intermediate arena; the output arena holds rs_h x rs_w x ncomp bytes per image
        b->rs_w = rs_w, b->rs_h = rs_h;
        b->pix_off = b->out_off, b->pix_len = b->out_len, b->pix_bytes = b->out_bytes;
        if (tensor) b->tn_es = tensor_elem_bytes(tensor->dtype), b->tn_flips.assign(n_images, 0);
        for (uint32_t i = 0; i < n_images; i++) lens[i] = (size_t)rs_w * rs_h * (rgb ? 3u : b->descs[i].ncomp) * (tensor ? b->tn_es : 1u);
        b->out_bytes = arena_layout(lens, b->out_off, b->out_len);
    }
    std::vector<size_t> wsrc_len;
    size_t wsrc_bytes = 0;
    if (b->warp) {  // (what the u8 batch's output arena would be)
        for (uint32_t i = 0; i < n_images; i++) lens[i] = (size_t)rs_w * rs_h * (rgb ? 3u : b->descs[i].ncomp);
        wsrc_bytes = arena_layout(lens, b->wsrc_off, wsrc_len);
    }

    {
        std::vector<uint32_t> keys;
        for (uint32_t i = 0; i < n_images; i++)
            if (kind_key[i] && std::find(keys.begin(), keys.end(), kind_key[i]) == keys.end()) keys.push_back(kind_key[i]);
        for (uint32_t key : keys) {
            std::vector<jpgpu_image_desc> sub;
            std::vector<uint32_t> ids;
            for (uint32_t i = 0; i < n_images; i++)
                if (kind_key[i] == key) {
                    sub.push_back(b->descs[i]);
                    ids.push_back(i);
                }
            FusedPlan fp;
            std::string why;
            if (!fused_plan(sub, ids, fp, why)) return set_err(b->err, JPGPU_ERR_INTERNAL, "fused plan: %s", why.c_str());
            b->fused.push_back(std::move(fp));
        }
        if (b->fused.empty()) b->path = b->generic_ids.empty() ? "" : "generic";
        else if (b->fused.size() == 1 && b->generic_ids.empty()) b->path = b->fused[0].name;
        else b->path = "mixed";
    }
    if (!b->scaled.empty()) b->path = (b->fused.empty() && b->generic_ids.empty()) ? b->scaled_name : "mixed";
    if (!b->win.empty()) b->path = b->path.empty() ? "window" : "mixed";
    if (b->path.empty()) b->path = "generic";
    if (rgb) b->path += "+rgb";
    if (b->placed) b->path += "+place";
    if (resized) b->path += "+resize";
    if (filter) b->path += std::string(":") + resample_filter_name(filter);
    if (b->warp) b->path += b->wp_filter == WP_BILINEAR ? "+warp:bilinear" : "+warp";
    if (tensor) b->path += "+tensor";
    const size_t full = arena_layout(b->out_full_len);  // (what the whole images take)
    if (!(flags & JPGPU_BATCH_EXTERNAL_BUFFERS)) {
        B_HIP(hipMalloc((void **)&b->d_coef, b->coef_bytes));
        b->own_coef = true;
        // (with windows: a quarter more than these need, at most what the whole images take — batch_rewindow sets other windows in place)
        b->out_cap = (b->win.empty() || resized) ? b->out_bytes : arena_headroom(b->out_bytes, full);
        B_HIP(hipMalloc((void **)&b->d_out, b->out_cap));
        b->own_out = true;
    }
    if (resized) {  // (the same headroom for other windows, in the intermediate arena)
        b->pix_cap = b->win.empty() ? b->pix_bytes : arena_headroom(b->pix_bytes, full);
        B_HIP(hipMalloc((void **)&b->d_pix, b->pix_cap));
        if (b->warp) {
            B_HIP(hipMalloc((void **)&b->d_wsrc, wsrc_bytes));
            B_HIP(hipMalloc((void **)&b->d_wp_jobs, warp_jobs_bytes(b)));
            b->wp_dirty = true;
        }
        const bool rs_tensor = tensor && !b->warp;  // (a warp: the resample's jobs are the u8 ones, the warp writes the tensor)
        if (tensor) {  // (the table of four channels: every image looks up its own first ncomp rows)
            B_HIP(hipMalloc(&b->d_tn_table, TN_TABLE_MAX));
            std::vector<uint32_t> table(TN_TABLE_MAX / 4u, 0u);
            uint32_t nc_max = rgb ? 3u : 1u;
            for (uint32_t i = 0; i < n_images && !rgb; i++) nc_max = std::max<uint32_t>(nc_max, b->descs[i].ncomp);
            tensor_table(tensor->dtype, tensor->mean, tensor->std, nc_max, table.data());
            B_HIP(hipMemcpy(b->d_tn_table, table.data(), TN_TABLE_MAX, hipMemcpyHostToDevice));
        }
        if (rs_tensor && b->placed) {
            B_HIP(hipMalloc((void **)&b->d_ptn_jobs, (size_t)n_images * sizeof(PlacedTensorJob)));
        } else if (rs_tensor) {
            B_HIP(hipMalloc((void **)&b->d_tn_jobs, (size_t)n_images * 2u * sizeof(TensorJob)));
        } else if (b->placed) {
            B_HIP(hipMalloc((void **)&b->d_pl_jobs, (size_t)n_images * sizeof(PlacedJob)));
        } else {
            B_HIP(hipMalloc((void **)&b->d_rs_jobs, (size_t)n_images * 2u * sizeof(ResampleJob)));
        }
        if (!b->placed) B_HIP(hipMalloc((void **)&b->d_rs_bpr, (size_t)n_images * sizeof(uint32_t)));
    }
    if (!b->generic_ids.empty()) B_HIP(hipMalloc((void **)&b->d_planes, b->plane_bytes_total));
    for (FusedPlan &fp : b->fused) {
        rc = fused_alloc(fp, b->err);
        if (rc) return rc;
        // no event per plan (a record per launch, a wait in fused_bind): b->enqueued stands behind the whole decode, and
        // batch_refresh_jobs waits for it before anything is rebound
        if (fp.launched) (void)hipEventDestroy(fp.launched);
        fp.launched = nullptr;
    }
    B_HIP(hipMalloc((void **)&b->d_qt, (size_t)n_images * 4 * 64 * sizeof(uint16_t)));
    rc = batch_upload_qt(b);
    if (rc) return rc;
    B_HIP(hipMalloc((void **)&b->d_plane_jobs, (size_t)n_images * 4 * sizeof(PlaneJob)));
    B_HIP(hipMalloc((void **)&b->d_image_jobs, (size_t)n_images * sizeof(ImageJob)));
    B_HIP(b->scaled.number_and_alloc(b->descs));
    B_HIP(b->win.number_and_alloc(b->descs));
    B_HIP(hipEventCreate(&b->ev0));
    B_HIP(hipEventCreate(&b->ev1));
    B_HIP(hipEventCreateWithFlags(&b->enqueued, hipEventDisableTiming));
    if (resized) return batch_resample_tables(b);
    return JPGPU_OK;
}

int jpgpu_batch_create(int device, const jpgpu_image_desc *descs, uint32_t n_images, uint32_t flags, jpgpu_batch **out) {
    return batch_create(device, descs, nullptr, 0, 0, nullptr, n_images, flags, out);
}
int jpgpu_batch_create_windowed(int device, const jpgpu_image_desc *descs, const jpgpu_window *windows, uint32_t n_images, uint32_t flags,
                                jpgpu_batch **out) {
    return batch_create(device, descs, windows, 0, 0, nullptr, n_images, flags, out);
}
int jpgpu_batch_create_resized(int device, const jpgpu_image_desc *descs, const jpgpu_window *windows, uint16_t out_w, uint16_t out_h,
                               uint32_t n_images, uint32_t flags, jpgpu_batch **out) {
    if (out_w == 0 || out_h == 0) {  // (0, 0 would mean "none" below: refuse it here)
        if (!out) return JPGPU_ERR_FORMAT;
        jpgpu_batch *b = new jpgpu_batch();
        *out = b;
        return set_err(b->err, JPGPU_ERR_FORMAT, "output size %ux%u: width and height must be 1..%u", out_w, out_h, RS_MAX_OUT);
    }
    return batch_create(device, descs, windows, out_w, out_h, nullptr, n_images, flags, out);
}
int jpgpu_batch_create_tensor(int device, const jpgpu_image_desc *descs, const jpgpu_window *windows, uint16_t out_w, uint16_t out_h,
                              const jpgpu_tensor_format *format, uint32_t n_images, uint32_t flags, jpgpu_batch **out) {
    if (out_w == 0 || out_h == 0 || !format) {  // (no output size, no format: refused here — below they would mean "none")
        if (!out) return JPGPU_ERR_FORMAT;
        jpgpu_batch *b = new jpgpu_batch();
        *out = b;
        if (!format) return set_err(b->err, JPGPU_ERR_FORMAT, "jpgpu_batch_create_tensor: no tensor format");
        return set_err(b->err, JPGPU_ERR_FORMAT, "a tensor format needs an output size (%ux%u: width and height must be 1..%u)", out_w, out_h, RS_MAX_OUT);
    }
    return batch_create(device, descs, windows, out_w, out_h, format, n_images, flags, out);
}
int jpgpu_batch_create_placed(int device, const jpgpu_image_desc *descs, const jpgpu_window *windows, const jpgpu_placement *placements,
                              const uint8_t *fill, uint16_t out_w, uint16_t out_h, const jpgpu_tensor_format *format, uint32_t n_images,
                              uint32_t flags, jpgpu_batch **out) {
    if (out_w == 0 || out_h == 0) {  // (0, 0 would mean "none" below: refuse it here)
        if (!out) return JPGPU_ERR_FORMAT;
        jpgpu_batch *b = new jpgpu_batch();
        *out = b;
        return set_err(b->err, JPGPU_ERR_FORMAT, "output size %ux%u: width and height must be 1..%u", out_w, out_h, RS_MAX_OUT);
    }
    return batch_create(device, descs, windows, out_w, out_h, format, n_images, flags, out, placements, fill);
}
int jpgpu_batch_set_flips(jpgpu_batch *b, const uint8_t *flips) {
    if (!b) return JPGPU_ERR_FORMAT;
    if (!b->tn_es) return set_err(b->err, JPGPU_ERR_UNSUPPORTED, "jpgpu_batch_set_flips: the batch has no tensor format");
    for (size_t i = 0; i < b->tn_flips.size(); i++) b->tn_flips[i] = flips && flips[i] ? 1 : 0;
    if (b->warp) b->wp_dirty = true;  // (a warped batch: the flip is a field of the WarpJobs)
    else b->tn_dirty = true;
    return JPGPU_OK;
}
int jpgpu_batch_create_warped(int device, const jpgpu_image_desc *descs, const jpgpu_window *windows, const jpgpu_placement *placements,
                              const uint8_t *fill, uint16_t out_w, uint16_t out_h, const jpgpu_tensor_format *format, const jpgpu_warp_options *warp,
                              uint32_t n_images, uint32_t flags, jpgpu_batch **out) {
    if (!warp) return jpgpu_batch_create_placed(device, descs, windows, placements, fill, out_w, out_h, format, n_images, flags, out);
    if (out_w == 0 || out_h == 0) {  // (0, 0 would mean "none" below: refuse it here)
        if (!out) return JPGPU_ERR_FORMAT;
        jpgpu_batch *b = new jpgpu_batch();
        *out = b;
        return set_err(b->err, JPGPU_ERR_FORMAT, "a warp needs an output size (%ux%u: width and height must be 1..%u)", out_w, out_h, RS_MAX_OUT);
    }
    return batch_create(device, descs, windows, out_w, out_h, format, n_images, flags, out, placements, fill, warp);
}
int jpgpu_batch_set_warps(jpgpu_batch *b, const jpgpu_warp *warps) {
    if (!b) return JPGPU_ERR_FORMAT;
    if (!b->warp) return set_err(b->err, JPGPU_ERR_UNSUPPORTED, "jpgpu_batch_set_warps: the batch has no warp (jpgpu_batch_create_warped)");
    for (size_t i = 0; warps && i < b->wp_m.size(); i++)  // (one refused matrix refuses the call: nothing is changed)
        if (!warp_check(warps[i].m, b->rs_w, b->rs_h))
            return set_err(b->err, JPGPU_ERR_FORMAT, "jpgpu_batch_set_warps: image %zu: matrix (%g, %g, %g, %g, %g, %g) refused for %ux%u (jpgpu_warp_check)", i,
                           warps[i].m[0], warps[i].m[1], warps[i].m[2], warps[i].m[3], warps[i].m[4], warps[i].m[5], b->rs_w, b->rs_h);
    for (size_t i = 0; i < b->wp_m.size(); i++) b->wp_m[i] = warps ? warps[i] : jpgpu_warp{{1.0, 0.0, 0.0, 0.0, 1.0, 0.0}};
    b->wp_dirty = true;
    return JPGPU_OK;
}
int jpgpu_warp_check(const jpgpu_warp *warp, uint32_t out_w, uint32_t out_h) {
    return (warp && out_w && out_h && warp_check(warp->m, out_w, out_h)) ? JPGPU_OK : JPGPU_ERR_FORMAT;
}
int jpgpu_warp_nearest_axis(double a, double b, uint32_t out_size, int32_t *idx) {
    if (!idx && out_size) return JPGPU_ERR_FORMAT;
    warp_nearest_axis(a, b, out_size, idx);
    return JPGPU_OK;
}

void jpgpu_batch_destroy(jpgpu_batch *b) {
    if (!b) return;
    std::string err;
    if (use_device(b->device, err) == JPGPU_OK) {
        hipDeviceSynchronize();
        if (b->own_coef && b->d_coef) hipFree(b->d_coef);
        if (b->own_out && b->d_out) hipFree(b->d_out);
        if (b->d_planes) hipFree(b->d_planes);
        if (b->d_pix) hipFree(b->d_pix);
        if (b->d_rs_jobs) hipFree(b->d_rs_jobs);
        if (b->d_rs_bpr) hipFree(b->d_rs_bpr);
        if (b->d_tn_jobs) hipFree(b->d_tn_jobs);
        if (b->d_pl_jobs) hipFree(b->d_pl_jobs);
        if (b->d_ptn_jobs) hipFree(b->d_ptn_jobs);
        if (b->h_ptn_jobs) hipHostFree(b->h_ptn_jobs);
        if (b->d_wsrc) hipFree(b->d_wsrc);
        if (b->d_wp_jobs) hipFree(b->d_wp_jobs);
        if (b->h_wp_jobs) hipHostFree(b->h_wp_jobs);
        if (b->wp_sent) hipEventDestroy(b->wp_sent);
        if (b->d_tn_table) hipFree(b->d_tn_table);
        if (b->h_tn_jobs) hipHostFree(b->h_tn_jobs);
        if (b->tn_sent) hipEventDestroy(b->tn_sent);
        if (b->d_rs_tab) hipFree(b->d_rs_tab);
        if (b->d_qt) hipFree(b->d_qt);
        if (b->d_compact) hipFree(b->d_compact);
        if (b->d_expand_jobs) hipFree(b->d_expand_jobs);
        if (b->h_expand_jobs) hipHostFree(b->h_expand_jobs);
        if (b->expand_sent) hipEventDestroy(b->expand_sent);
        if (b->d_entropy) hipFree(b->d_entropy);
        if (b->h_entropy) hipHostFree(b->h_entropy);
        if (b->h_entropy_out) hipHostFree(b->h_entropy_out);
        if (b->entropy_uploaded) hipEventDestroy(b->entropy_uploaded);
        if (b->entropy_filled) hipEventDestroy(b->entropy_filled);
        if (b->h_bounce) hipHostFree(b->h_bounce);
        if (b->d_scan) hipFree(b->d_scan);
        if (b->h_scan) hipHostFree(b->h_scan);
        if (b->d_stats) hipFree(b->d_stats);
        if (b->d_host_cls) hipFree(b->d_host_cls);
        if (b->h_host_cls) hipHostFree(b->h_host_cls);
        if (b->d_plane_job_slot) hipFree(b->d_plane_job_slot);
        for (auto &e : b->cls_sent)
            if (e) hipEventDestroy(e);
        for (auto &e : b->ev_phase)
            if (e) hipEventDestroy(e);
        if (b->d_plane_jobs) hipFree(b->d_plane_jobs);
        if (b->d_image_jobs) hipFree(b->d_image_jobs);
        b->scaled.free();
        b->win.free();
        for (FusedPlan &fp : b->fused) fused_free(fp);
        if (b->ev0) hipEventDestroy(b->ev0);
        if (b->ev1) hipEventDestroy(b->ev1);
        if (b->enqueued) hipEventDestroy(b->enqueued);
    }
    delete b;
}

const char *jpgpu_batch_last_error(const jpgpu_batch *b) { return b ? b->err.c_str() : ""; }
const char *jpgpu_batch_path(const jpgpu_batch *b) { return b ? b->path.c_str() : ""; }
int jpgpu_batch_class_counts(jpgpu_batch *b, uint32_t counts[3]) {
    if (!b || !counts) return JPGPU_ERR_FORMAT;
    int rc = use_device(b->device, b->err);
    if (rc) return rc;
    B_HIP(batch_wait_enqueued(b));  // (the refresh below sends on the null stream)
    rc = batch_refresh_jobs(b);
    if (rc) return rc;
    counts[0] = counts[1] = counts[2] = 0;
    if (b->dev_classes) {  // the classes live on the device: have them worked out there and read the image tables back
        B_HIP(hipDeviceSynchronize());
        for (FusedPlan &fp : b->fused) {
            B_HIP(fused_finalize_classes(fp, nullptr, b->d_stats, b->d_host_cls));
            std::vector<uint8_t> bits;
            rc = fused_read_classes(fp, bits, b->err);
            if (rc) return rc;
            for (uint8_t f : bits) counts[(f & 2u) ? 2 : ((f & 1u) ? 1 : 0)]++;
        }
        return JPGPU_OK;
    }
    for (const FusedPlan &fp : b->fused)
        for (int c = 0; c < 3; c++) counts[c] += fp.class_images[c];
    return JPGPU_OK;
}
size_t jpgpu_batch_coef_arena_bytes(const jpgpu_batch *b) { return b ? b->coef_bytes : 0; }
size_t jpgpu_batch_out_arena_bytes(const jpgpu_batch *b) { return b ? b->out_bytes : 0; }
size_t jpgpu_batch_coef_offset(const jpgpu_batch *b, uint32_t image, uint32_t comp) {
    return (b && image < b->descs.size() && comp < 4) ? b->coef_off[image * 4 + comp] : 0;
}
size_t jpgpu_batch_coef_bytes(const jpgpu_batch *b, uint32_t image, uint32_t comp) {
    return (b && image < b->descs.size() && comp < 4) ? b->coef_len[image * 4 + comp] : 0;
}
size_t jpgpu_batch_out_offset(const jpgpu_batch *b, uint32_t image) {
    return (b && image < b->descs.size()) ? b->out_off[image] : 0;
}
size_t jpgpu_batch_out_bytes(const jpgpu_batch *b, uint32_t image) {
    return (b && image < b->descs.size()) ? b->out_len[image] : 0;
}
void *jpgpu_batch_coef_arena(const jpgpu_batch *b) { return b ? b->d_coef : nullptr; }
void *jpgpu_batch_out_arena(const jpgpu_batch *b) { return b ? b->d_out : nullptr; }

int jpgpu_batch_bind(jpgpu_batch *b, void *device_coef_arena, void *device_out_arena) {
    if (!b) return JPGPU_ERR_FORMAT;
    if (!(b->flags & JPGPU_BATCH_EXTERNAL_BUFFERS)) return set_err(b->err, JPGPU_ERR_FORMAT, "batch owns its buffers");
    if (!device_coef_arena || !device_out_arena || ((uintptr_t)device_coef_arena & 255) || ((uintptr_t)device_out_arena & 255))
        return set_err(b->err, JPGPU_ERR_FORMAT, "bind: arenas must be non-null and 256-byte aligned");
    b->d_coef = (uint8_t *)device_coef_arena;
    b->d_out = (uint8_t *)device_out_arena;
    b->jobs_dirty = true;
    b->scan_jobs_valid = false;
    return JPGPU_OK;
}

int jpgpu_batch_set_range_hint(jpgpu_batch *b, uint32_t image, int sane) {
    if (!b || image >= b->descs.size()) return JPGPU_ERR_FORMAT;
    for (uint32_t c = 0; c < 4; c++) batch_set_host_class(b, (size_t)image * 4 + c, (uint8_t)(sane & 3));
    return JPGPU_OK;
}

int jpgpu_batch_set_range_class(jpgpu_batch *b, uint32_t image, uint32_t comp, int range_class) {
    if (!b || image >= b->descs.size() || comp >= 4) return JPGPU_ERR_FORMAT;
    batch_set_host_class(b, (size_t)image * 4 + comp, (uint8_t)(range_class & 3));
    return JPGPU_OK;
}

// the range-scan job table on the device (d_scan: [ stats of the blocking scan | RangeJob[] ]); slot = image * 4 + comp
static int batch_scan_jobs(jpgpu_batch *b, uint32_t &n_jobs, uint32_t &max_blocks, size_t &jobs_off) {
    const size_t n_jobs_max = b->descs.size() * 4;
    const size_t stats_bytes = b->descs.size() * 4 * RS_WORDS * sizeof(uint32_t);
    jobs_off = align_up(stats_bytes, 256);
    if (!b->d_scan) {
        B_HIP(hipMalloc((void **)&b->d_scan, jobs_off + 2 * n_jobs_max * sizeof(RangeJob)));
        B_HIP(hipHostMalloc((void **)&b->h_scan, stats_bytes, hipHostMallocDefault));
        b->scan_jobs_valid = false;
    }
    max_blocks = 0, n_jobs = 0;
    for (size_t i = 0; i < b->descs.size(); i++)
        for (uint32_t c = 0; c < b->descs[i].ncomp; c++) {
            max_blocks = std::max(max_blocks, (uint32_t)(b->coef_len[i * 4 + c] / 128));
            n_jobs++;
        }
    if (!b->scan_jobs_valid) {
        // two tables back to back: slots per component (the blocking scan's per-component classes) and per image (the
        // device-side statistics are kept per image: range_stats.hpp)
        std::vector<RangeJob> jobs;
        for (int per_image = 0; per_image < 2; per_image++)
            for (size_t i = 0; i < b->descs.size(); i++)
                for (uint32_t c = 0; c < b->descs[i].ncomp; c++) {
                    RangeJob r;
                    r.coefs = reinterpret_cast<const int16_t *>(b->d_coef + b->coef_off[i * 4 + c]);
                    r.n_blocks = (uint32_t)(b->coef_len[i * 4 + c] / 128);
                    r.slot = per_image ? (uint32_t)i : (uint32_t)(i * 4 + c);
                    memcpy(r.q, b->descs[i].quantization_tables[c], 128);
                    jobs.push_back(r);
                }
        B_HIP(batch_wait_enqueued(b));  // (a scan of jpgpu_batch_classify_on_device still queued reads the table)
        B_HIP(hipMemcpy(b->d_scan + jobs_off, jobs.data(), jobs.size() * sizeof(RangeJob), hipMemcpyHostToDevice));
        b->scan_jobs_valid = true;
    }
    return JPGPU_OK;
}

static int batch_expand_pending(jpgpu_batch *b, hipStream_t s);

// Compact uploads reach the arena at the next decode; a pass that classifies "the coefficients as they stand in the arena" expands
// them first, or it would classify what the images held before (tables first: the expansion ranges unclassified uploads with them)
static int batch_settle_arena(jpgpu_batch *b, hipStream_t s) {
    int rc = batch_refresh_jobs(b, s);
    if (rc) return rc;
    return batch_expand_pending(b, s);
}

int jpgpu_batch_scan_ranges(jpgpu_batch *b, void *hip_stream, uint8_t *classes) {
    if (!b) return JPGPU_ERR_FORMAT;
    int rc = use_device(b->device, b->err);
    if (rc) return rc;
    if (!b->d_coef) return set_err(b->err, JPGPU_ERR_FORMAT, "batch has no device buffers bound");
    hipStream_t s = (hipStream_t)hip_stream;
    rc = batch_settle_arena(b, s);
    if (rc) return rc;
    // stats and job table live on the device between calls (a call per decode must not allocate: bench.py times it)
    uint32_t max_blocks = 0, n_jobs = 0;
    size_t jobs_off = 0;
    rc = batch_scan_jobs(b, n_jobs, max_blocks, jobs_off);
    if (rc) return rc;
    const size_t stats_bytes = b->descs.size() * 4 * RS_WORDS * sizeof(uint32_t);
    uint32_t *stats = b->h_scan;
    hipError_t e = hipMemsetAsync(b->d_scan, 0, stats_bytes, s);
    if (e == hipSuccess)
        e = launch_range_scan(reinterpret_cast<const RangeJob *>(b->d_scan + jobs_off), n_jobs, max_blocks, reinterpret_cast<uint32_t *>(b->d_scan), s);
    if (e == hipSuccess) e = hipMemcpyAsync(stats, b->d_scan, stats_bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return set_err(b->err, JPGPU_ERR_IO, "scan_ranges: %s", hipGetErrorString(e));
    for (size_t i = 0; i < b->descs.size(); i++)
        for (uint32_t c = 0; c < 4; c++) {
            uint8_t cls = 0;
            if (c < b->descs[i].ncomp) {
                const uint32_t *st = stats + (i * 4 + c) * RS_WORDS;
                cls = (uint8_t)range_class_from_stats(st[RS_MAX_DC], st[RS_MAX_AC], st[RS_MAX_COL], 1u);
                batch_set_host_class(b, i * 4 + c, cls);
            }
            if (classes) classes[i * 4 + c] = cls;
        }
    return JPGPU_OK;
}

int jpgpu_batch_classify_on_device(jpgpu_batch *b, void *hip_stream) {
    if (!b) return JPGPU_ERR_FORMAT;
    int rc = use_device(b->device, b->err);
    if (rc) return rc;
    if (!b->d_coef) return set_err(b->err, JPGPU_ERR_FORMAT, "batch has no device buffers bound");
    hipStream_t s = (hipStream_t)hip_stream;
    rc = batch_enable_dev_classes(b);
    if (rc) return rc;
    rc = batch_settle_arena(b, s);
    if (rc) return rc;
    batch_drop_entries(b);  // (the caller declares the arena the images' source)
    uint32_t max_blocks = 0, n_jobs = 0;
    size_t jobs_off = 0;
    rc = batch_scan_jobs(b, n_jobs, max_blocks, jobs_off);
    if (rc) return rc;
    // zero, then the scan (which also marks the column maxima as exact: RS_COL_EXACT)
    B_HIP(hipMemsetAsync(b->d_stats, 0, b->descs.size() * RS_WORDS * sizeof(uint32_t), s));
    B_HIP(launch_range_scan(reinterpret_cast<const RangeJob *>(b->d_scan + jobs_off) + n_jobs, n_jobs, max_blocks, b->d_stats, s));
    for (size_t i = 0; i < b->descs.size(); i++)
        for (uint32_t c = 0; c < b->descs[i].ncomp; c++) {
            b->sane[i * 4 + c] = 0;  // (the host does not know)
            batch_class_source(b, i * 4 + c, true);
        }
    B_HIP(batch_mark_enqueued(b, s));  // (the scan reads its job table and the coefficient arena)
    return JPGPU_OK;
}

int jpgpu_batch_set_quantization_table(jpgpu_batch *b, uint32_t image, uint32_t comp, const uint16_t q[64]) {
    if (!b || !q || image >= b->descs.size() || comp >= b->descs[image].ncomp) return JPGPU_ERR_FORMAT;
    if (memcmp(b->descs[image].quantization_tables[comp], q, 128) == 0) return JPGPU_OK;
    memcpy(b->descs[image].quantization_tables[comp], q, 128);
    // the range class of coefficients already uploaded was computed with the old table (|c*q| bounds): unknown again
    // (statistics the device gathered with the old table included)
    batch_set_host_class(b, (size_t)image * 4 + comp, 0);
    b->scan_jobs_valid = false;
    b->qt_dirty = true;
    b->jobs_dirty = true;
    return JPGPU_OK;
}

int jpgpu_batch_upload(jpgpu_batch *b, uint32_t image, uint32_t comp, const int16_t *coefficients, size_t len) {
    if (!b) return JPGPU_ERR_FORMAT;
    if (image >= b->descs.size() || comp >= b->descs[image].ncomp || !coefficients)
        return set_err(b->err, JPGPU_ERR_FORMAT, "upload: bad image/component");
    if (len * sizeof(int16_t) != b->coef_len[image * 4 + comp])
        return set_err(b->err, JPGPU_ERR_FORMAT, "upload: %zu coefficients, geometry needs %zu", len,
                       b->coef_len[image * 4 + comp] / sizeof(int16_t));
    int rc = use_device(b->device, b->err);
    if (rc) return rc;
    if (!b->d_coef) return set_err(b->err, JPGPU_ERR_FORMAT, "batch has no device buffers bound");
    // range scan (part of H2D staging): per-position max |c| times q must stay below 2^15 for
    // the 24-bit multiply path to be exact (pixel_math.hpp idct8x8<SANE>)
    uint8_t sane = 0;  // bit0: every |c*q| < 2^15; bit1: additionally every column sum of |c*q| <= 5900
    if (!(b->flags & JPGPU_BATCH_ASSUME_HOSTILE))
        sane = (uint8_t)jpgpu_range_class(coefficients, len, b->descs[image].quantization_tables[comp]);
    batch_set_host_class(b, (size_t)image * 4 + comp, sane);
    {
        // a compact upload of this component still waiting for its expansion is superseded: the last upload before a decode wins
        std::lock_guard<std::mutex> g(b->compact_mutex);
        if (!b->compact_pending.empty()) b->compact_pending[(size_t)image * 4 + comp] = 0;
    }
    B_HIP(batch_wait_enqueued(b));  // (a decode still queued reads the coefficients this copy replaces)
    B_HIP(hipMemcpy(b->d_coef + b->coef_off[image * 4 + comp], coefficients, len * sizeof(int16_t), hipMemcpyHostToDevice));
    return JPGPU_OK;
}

}  // extern "C"

// `trusted`: the buffer comes from CompactWriter in this library (pipeline.cpp) — skip the consistency pass
int jpgpu::batch_upload_compact(jpgpu_batch *b, uint32_t image, uint32_t comp, const void *compact, size_t bytes,
                                int range_class, void *hip_stream, bool trusted) {
    if (!b) return JPGPU_ERR_FORMAT;
    if (image >= b->descs.size() || comp >= b->descs[image].ncomp || !compact)
        return set_err(b->err, JPGPU_ERR_FORMAT, "upload_compact: bad image/component");
    const size_t idx = (size_t)image * 4 + comp, nblk = b->coef_len[idx] / 128;
    // the device trusts the index: check it here (one pass over the fixed part)
    if (bytes < nblk * 12 || ((bytes - nblk * 12) & 1) || bytes > compact_max_bytes(nblk))
        return set_err(b->err, JPGPU_ERR_FORMAT, "upload_compact: %zu bytes do not fit %zu blocks", bytes, nblk);
    if (!trusted) {
        const uint64_t *bm = static_cast<const uint64_t *>(compact);
        const uint32_t *first = reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(compact) + nblk * 8);
        size_t n = 0;
        for (size_t k = 0; k < nblk; k++) {
            if (first[k] != n) return set_err(b->err, JPGPU_ERR_FORMAT, "upload_compact: inconsistent value index at block %zu", k);
            n += (size_t)__builtin_popcountll(bm[k]);
        }
        if (n * 2 != bytes - nblk * 12) return set_err(b->err, JPGPU_ERR_FORMAT, "upload_compact: value count does not match the bitmaps");
    }
    int rc = use_device(b->device, b->err);
    if (rc) return rc;
    if (!b->d_coef) return set_err(b->err, JPGPU_ERR_FORMAT, "batch has no device buffers bound");
    {
        std::lock_guard<std::mutex> g(b->compact_mutex);
        if (!b->d_compact) {
            const size_t n = b->descs.size();
            b->compact_off.assign(n * 4, 0);
            b->compact_pending.assign(n * 4, 0);
            size_t off = 0;
            for (size_t i = 0; i < n; i++)
                for (uint32_t c = 0; c < b->descs[i].ncomp; c++) {
                    b->compact_off[i * 4 + c] = off;
                    off += align_up(compact_max_bytes(b->coef_len[i * 4 + c] / 128), 256);
                }
            B_HIP(hipMalloc((void **)&b->d_compact, std::max<size_t>(off, 256)));
            B_HIP(hipMalloc((void **)&b->d_expand_jobs, n * 4 * sizeof(ExpandJob)));
            B_HIP(hipHostMalloc((void **)&b->h_expand_jobs, n * 4 * sizeof(ExpandJob), hipHostMallocDefault));
            B_HIP(hipEventCreateWithFlags(&b->expand_sent, hipEventDisableTiming));
        }
        // range_class < 0: the sender did not classify — expand_compact_kernel ranges the values while it expands them
        b->compact_pending[idx] = range_class >= 0 ? 1 : 2;
        b->any_compact_pending = true;
        if (range_class >= 0) {
            batch_set_host_class(b, idx, (uint8_t)(range_class & 3));
        } else {
            rc = batch_enable_dev_classes(b);
            if (rc) return rc;
            batch_drop_entry_image(b, image);  // (what batch_set_host_class does in the other branch)
            b->sane[idx] = 0;
            // (the whole plane is replaced and ranged, at expansion time, with the table the device then holds — batch_refresh_jobs
            // runs first; older maxima only over-estimate)
            batch_class_source(b, idx, true);
        }
    }
    B_HIP(hipMemcpyAsync(b->d_compact + b->compact_off[idx], compact, bytes, hipMemcpyHostToDevice, (hipStream_t)hip_stream));
    return JPGPU_OK;
}

int jpgpu::copy_device_to_pinned_host(void *host_pinned, const void *d_src, size_t bytes, void *hip_stream) {
    static const bool engine = getenv("JPGPU_DOWNLOAD_BY_COPY_ENGINE") != nullptr;  // A/B: hipMemcpyAsync instead of the copy kernel
    void *mapped = nullptr;
    if (!engine && ((uintptr_t)host_pinned & 15u) == 0 && ((uintptr_t)d_src & 15u) == 0 && hipHostGetDevicePointer(&mapped, host_pinned, 0) == hipSuccess)
        return launch_copy_to_host(mapped, d_src, bytes, (hipStream_t)hip_stream) == hipSuccess ? JPGPU_OK : JPGPU_ERR_IO;
    (void)hipGetLastError();
    return hipMemcpyAsync(host_pinned, d_src, bytes, hipMemcpyDeviceToHost, (hipStream_t)hip_stream) == hipSuccess ? JPGPU_OK : JPGPU_ERR_IO;
}

// What jpgpu_batch_create_windowed would make of window `wn` on an image of descriptor `d`, without a batch (window_rule,
// batch_layout.hpp): the pipeline sorts images out one by one before it forms sub-batches (a batch fails creation as a whole).
int jpgpu::batch_check_window(const jpgpu_image_desc &d, const jpgpu_window &wn, bool &windowed, uint32_t &gw, uint32_t &gh, std::string &why) {
    WindowGeom wg;
    return window_rule(d, wn, windowed, gw, gh, wg, why);
}
// Other windows for the SAME window group (the pipeline's kept sub-batches; the batch must be idle): only the group's geometry, the
// output offsets / sizes and the job tables depend on the windows — the coefficient arena, the fused plans' membership and every
// staging block stay.  JPGPU_ERR_UNSUPPORTED, with nothing changed, when another set of images would be windowed (or the buffers
// are the caller's): the caller creates a new batch then.  The output arena grows when the new windows need more than it holds.
// `placements` (a placed batch; NULL: those it has): set with the windows.  A batch is placed or not for its lifetime — other device
// job records, another launch — so placements for a batch without any, or none that differs from the whole output for a placed
// one, are JPGPU_ERR_UNSUPPORTED too; one that shows no pixel is JPGPU_ERR_FORMAT.  Nothing is changed then.
int jpgpu::batch_rewindow(jpgpu_batch *b, const jpgpu_window *windows, const jpgpu_placement *placements) {
    if (!b || !windows) return JPGPU_ERR_FORMAT;
    if ((!b->own_out && !b->rs_w) || b->win.empty()) return JPGPU_ERR_UNSUPPORTED;  // (with an output size the windows' bytes are the batch's own)
    std::vector<jpgpu_placement> pls;
    if (placements) {
        bool any = false;
        pls.assign(placements, placements + b->descs.size());
        for (jpgpu_placement &pl : pls) {
            if (pl.rw == 0 || pl.rh == 0) pl = jpgpu_placement{(uint16_t)b->rs_w, (uint16_t)b->rs_h, 0, 0};
            uint32_t first, count, v0;
            if (!placed_axis(pl.rw, pl.x, b->rs_w, first, count, v0) || !placed_axis(pl.rh, pl.y, b->rs_h, first, count, v0)) return JPGPU_ERR_FORMAT;
            any = any || pl.rw != b->rs_w || pl.rh != b->rs_h || pl.x != 0 || pl.y != 0;
        }
        if (any != b->placed) return JPGPU_ERR_UNSUPPORTED;
    }
    std::vector<WindowGeom> geoms;
    std::vector<size_t> lens;
    int rc = window_rule_rewindow(b->descs, b->win.ids, b->out_full_len, windows, geoms, lens);
    if (rc) return rc;
    rc = use_device(b->device, b->err);
    if (rc) return rc;
    // (with an output size the windows' bytes live in the intermediate arena: the resized arena never changes)
    size_t &w_bytes = b->rs_w ? b->pix_bytes : b->out_bytes, &w_cap = b->rs_w ? b->pix_cap : b->out_cap;
    uint8_t *&w_arena = b->rs_w ? b->d_pix : b->d_out;
    w_bytes = b->rs_w ? arena_layout(lens, b->pix_off, b->pix_len) : arena_layout(lens, b->out_off, b->out_len);
    b->jobs_dirty = true;  // (every job's output pointer, the fused plans' included)
    B_HIP(batch_wait_enqueued(b));  // (idle by contract: the event has completed)
    if (w_bytes > w_cap) {
        B_HIP(hipDeviceSynchronize());
        B_HIP(grow_device(w_arena, w_cap, w_bytes, arena_headroom(w_bytes, arena_layout(b->out_full_len))));
    }
    B_HIP(b->win.set_geoms(geoms, b->descs));
    if (b->placed && placements) b->pl = pls;
    if (b->rs_w) return batch_resample_tables(b);
    return JPGPU_OK;
}
// bytes the output arena of the batch would hold without any window (what a pinned copy of it never needs more than)
size_t jpgpu::batch_out_arena_bound(const jpgpu_batch *b) {
    if (b && b->rs_w) return b->out_bytes;  // (an output size: the arena never changes)
    return arena_layout(b ? b->out_full_len : std::vector<size_t>());
}
bool jpgpu::batch_image_windowed(const jpgpu_batch *b, uint32_t image) {
    return b && std::binary_search(b->win.ids.begin(), b->win.ids.end(), image);  // (win.ids is filled in image order)
}
uint32_t jpgpu::batch_windowed_images(const jpgpu_batch *b) { return b ? (uint32_t)b->win.ids.size() : 0u; }


extern "C" {

int jpgpu_batch_upload_compact(jpgpu_batch *b, uint32_t image, uint32_t comp, const void *compact, size_t bytes,
                               int range_class, void *hip_stream) {
    return jpgpu::batch_upload_compact(b, image, comp, compact, bytes, range_class, hip_stream, false);
}

// compact uploads since the last decode -> dense coefficient arena, on the decode stream
static int batch_expand_pending(jpgpu_batch *b, hipStream_t s) {
    std::vector<ExpandJob> jobs;
    std::vector<uint32_t> stat_fresh;
    uint32_t max_blocks = 0;
    {
        std::lock_guard<std::mutex> g(b->compact_mutex);
        if (!b->any_compact_pending) return JPGPU_OK;
        // An image's statistics start afresh when every component they stand for is being re-sent now; otherwise they only
        // grow (sound, possibly pessimistic).
        for (size_t img = 0; img < b->descs.size(); img++) {
            bool any = false, all = true;
            for (uint32_t c = 0; c < b->descs[img].ncomp; c++) {
                const size_t idx = img * 4 + c;
                if (b->compact_pending[idx] == 2 && b->cls_src[idx]) any = true;
                else if (b->cls_src[idx]) all = false;
            }
            if (any && all) stat_fresh.push_back((uint32_t)img);
        }
        for (size_t idx = 0; idx < b->compact_pending.size(); idx++)
            if (b->compact_pending[idx]) {
                ExpandJob j{};
                j.compact = b->d_compact + b->compact_off[idx];
                j.dense = reinterpret_cast<int16_t *>(b->d_coef + b->coef_off[idx]);
                j.n_blocks = (uint32_t)(b->coef_len[idx] / 128);
                if (b->compact_pending[idx] == 2 && b->cls_src[idx]) {  // unclassified by the sender: ranged on the way
                    j.qt = b->d_qt + idx * 64;
                    j.stats = b->d_stats + (idx / 4) * RS_WORDS;
                }
                max_blocks = std::max(max_blocks, j.n_blocks);
                jobs.push_back(j);
                b->compact_pending[idx] = 0;
            }
        b->any_compact_pending = false;
    }
    if (jobs.empty()) return JPGPU_OK;
    for (uint32_t img : stat_fresh) B_HIP(hipMemsetAsync(b->d_stats + (size_t)img * RS_WORDS, 0, RS_WORDS * sizeof(uint32_t), s));
    // The jobs follow the expansion before them on its own stream (a blocking copy on the null stream could overtake it on a non-blocking
    // stream, and would hold every decode of a loader up); the mirror is free once its last copy has left it.
    B_HIP(hipEventSynchronize(b->expand_sent));
    memcpy(b->h_expand_jobs, jobs.data(), jobs.size() * sizeof(ExpandJob));
    B_HIP(hipMemcpyAsync(b->d_expand_jobs, b->h_expand_jobs, jobs.size() * sizeof(ExpandJob), hipMemcpyHostToDevice, s));
    B_HIP(hipEventRecord(b->expand_sent, s));
    B_HIP(launch_expand_compact(b->d_expand_jobs, (uint32_t)jobs.size(), max_blocks, s));
    return JPGPU_OK;
}

int jpgpu_batch_decode(jpgpu_batch *b, void *hip_stream) {
    if (!b) return JPGPU_ERR_FORMAT;
    jpgpu::TraceRange roctx_range("jpgpu_batch_decode");
    int rc = use_device(b->device, b->err);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    rc = batch_refresh_jobs(b, s);
    if (rc) return rc;
    rc = batch_expand_pending(b, s);
    if (rc) return rc;
    if (b->phase_events_valid) B_HIP(hipEventRecord(b->ev_phase[4], s));
    // device-side classes: statistics -> class bits in the launch tables (class_finalize_*), then the `_dyn` kernels
    const uint32_t *st = b->dev_classes ? b->d_stats : nullptr;
    const uint8_t *hc = b->dev_classes ? b->d_host_cls : nullptr;
    auto entry_images_of = [&](const FusedPlan &fp) {
        uint32_t e = 0;
        if (fp.kind == FUSED_420 && fp.strip && !b->entry_img.empty())
            for (uint32_t id : fp.ids) e += b->entry_img[id];
        return e;
    };
    if (b->entries_pending) {  // the walk that reads the entry lists of the launch in front of this decode, and what it flagged
        b->entries_pending = false;
        for (FusedPlan &fp : b->fused)
            if (entry_images_of(fp)) B_HIP(fused_launch_entries(fp, s, b->d_entry_srcs));
        B_HIP(batch_status_to_host(b, b->d_entry_status, b->entry_status_n, s));
    }
    for (FusedPlan &fp : b->fused)
        if (entry_images_of(fp) < fp.n_images) B_HIP(fused_launch(fp, s, st, hc));  // (a plan of entry-list images only has nothing for the dense kernels)
    if (!b->scaled.empty())
        B_HIP(launch_scaled_fused(b->scaled.d_geoms, b->scaled.d_image_jobs, b->scaled.d_plane_jobs, (uint32_t)b->scaled.ids.size(), b->scaled.max_tiles_x,
                                  b->scaled.max_bands, b->scaled.lds_bytes, b->scaled.scales, s));
    if (!b->generic_ids.empty()) {
        const uint32_t n = (uint32_t)b->image_jobs.size();
        if (b->dev_classes) B_HIP(launch_class_finalize_planes(b->d_plane_jobs, b->d_plane_job_slot, (uint32_t)b->plane_jobs.size(), st, hc, s));
        static const uint32_t kScales[4] = {8, 4, 2, 1};
        for (uint32_t sc : kScales)
            if (b->scales[sc]) B_HIP(launch_idct_planes(b->d_plane_jobs, (uint32_t)b->plane_jobs.size(), b->max_blocks, sc, s));
        B_HIP(launch_upsample_color(b->d_image_jobs, n, b->max_w, b->max_h, s));
    }
    if (!b->win.empty())  // (windows: after the others)
        B_HIP(launch_window_band(b->win.d_geoms, b->win.d_image_jobs, b->win.d_plane_jobs, (uint32_t)b->win.ids.size(), b->win.max_tiles_x, b->win.max_bands,
                                 b->win.lds_bytes, b->win.scales, s));
    if (b->tn_es && b->tn_sent) B_HIP(hipStreamWaitEvent(s, b->tn_sent, 0));  // (the jobs may have gone up on another stream than this one)
    const bool rgb_out = (b->flags & JPGPU_BATCH_RGB_OUTPUT) != 0;
    const bool rs_tensor = b->tn_es && !b->warp;  // (a warped batch resamples to u8, whatever it writes in the end)
    if (b->placed && rs_tensor)  // (placements: the kernels of placed.hip, for this batch only)
        B_HIP(launch_resample_placed_tensor(b->d_ptn_jobs, b->d_rs_tab, b->d_tn_table, b->tn_es, (uint32_t)b->descs.size(), b->rs_max_bands, b->rs_lds_bytes, s, rgb_out));
    else if (b->placed)
        B_HIP(launch_resample_placed(b->d_pl_jobs, b->d_rs_tab, (uint32_t)b->descs.size(), b->rs_max_bands, b->rs_lds_bytes, s, rgb_out));
    else if (rs_tensor)  // (a tensor output: the same resample, its vertical pass writes every image's tensor)
        B_HIP(launch_resample_tensor(b->d_tn_jobs, b->d_rs_tab, b->d_tn_table, b->tn_es, (uint32_t)b->descs.size(), b->rs_max_bands, b->rs_lds_bytes, s,
                                      (b->flags & JPGPU_BATCH_RGB_OUTPUT) != 0));
    else if (b->rs_w)  // (an output size: every image's pixels, wherever the launches above left them in the intermediate arena)
        B_HIP(launch_resample_band(b->d_rs_jobs, b->d_rs_tab, (uint32_t)b->descs.size(), b->rs_max_bands, b->rs_lds_bytes, s, (b->flags & JPGPU_BATCH_RGB_OUTPUT) != 0));
    if (b->rs_max_runs && !b->placed) {  // (the images whose bands go in runs: their own launch, beside the band launch above)
        const uint32_t n_rs = (uint32_t)b->descs.size();
        if (rs_tensor) B_HIP(launch_resample_tensor_run(b->d_tn_jobs + n_rs, b->d_rs_tab, b->d_tn_table, b->d_rs_bpr, b->tn_es, n_rs, b->rs_max_runs, b->rs_lds_bytes, s));
        else B_HIP(launch_resample_run(b->d_rs_jobs + n_rs, b->d_rs_tab, b->d_rs_bpr, n_rs, b->rs_max_runs, b->rs_lds_bytes, s));
    }
    if (b->warp) {  // (the warp: behind the resample on the same stream, from the second intermediate arena into the output arena)
        const uint32_t tiles = (b->rs_w * b->rs_h + WP_NT - 1u) / WP_NT;
        const int32_t *tabs = reinterpret_cast<const int32_t *>(b->d_wp_jobs + b->descs.size() * sizeof(WarpJob));
        if (b->wp_sent) B_HIP(hipStreamWaitEvent(s, b->wp_sent, 0));  // (the jobs may have gone up on another stream than this one)
        B_HIP(launch_warp(reinterpret_cast<const WarpJob *>(b->d_wp_jobs), tabs, b->d_tn_table, b->tn_es, (uint32_t)b->descs.size(), tiles, s));
    }
    if (b->phase_events_valid) B_HIP(hipEventRecord(b->ev_phase[5], s));
    B_HIP(batch_mark_enqueued(b, s));
    return JPGPU_OK;
}

int jpgpu_batch_synchronize(jpgpu_batch *b, void *hip_stream) {
    if (!b) return JPGPU_ERR_FORMAT;
    int rc = use_device(b->device, b->err);
    if (rc) return rc;
    B_HIP(hipStreamSynchronize((hipStream_t)hip_stream));
    return JPGPU_OK;
}

int jpgpu_batch_download(jpgpu_batch *b, uint32_t image, uint8_t *dst, size_t cap, size_t *len) {
    if (!b) return JPGPU_ERR_FORMAT;
    if (image >= b->descs.size()) return set_err(b->err, JPGPU_ERR_FORMAT, "download: bad image");
    const size_t n = b->out_len[image];
    if (len) *len = n;
    if (!dst || cap < n) return set_err(b->err, JPGPU_ERR_FORMAT, "download: destination too small");
    int rc = use_device(b->device, b->err);
    if (rc) return rc;
    if (!b->d_out) return set_err(b->err, JPGPU_ERR_FORMAT, "batch has no device buffers bound");
    B_HIP(hipDeviceSynchronize());
    if (n == 0) return JPGPU_OK;
    // straight into pageable memory the copy runs at 0.5 GB/s (the runtime pins the destination page by page): bounce
    // through pinned memory unless the caller's buffer is pinned itself
    hipPointerAttribute_t attr;
    const bool pinned = hipPointerGetAttributes(&attr, dst) == hipSuccess && attr.type == hipMemoryTypeHost;
    if (!pinned) (void)hipGetLastError();
    if (pinned || n < (64u << 10)) {
        B_HIP(hipMemcpy(dst, b->d_out + b->out_off[image], n, hipMemcpyDeviceToHost));
        return JPGPU_OK;
    }
    if (b->h_bounce_cap < n) B_HIP(grow_pinned(b->h_bounce, b->h_bounce_cap, n));
    B_HIP(hipMemcpy(b->h_bounce, b->d_out + b->out_off[image], n, hipMemcpyDeviceToHost));
    memcpy(dst, b->h_bounce, n);
    return JPGPU_OK;
}

int jpgpu_batch_time(jpgpu_batch *b, void *hip_stream, uint32_t iters, float *ms_per_decode) {
    if (!b || !ms_per_decode || iters == 0) return JPGPU_ERR_FORMAT;
    int rc = use_device(b->device, b->err);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    rc = jpgpu_batch_decode(b, hip_stream);  // warm-up + job upload
    if (rc) return rc;
    B_HIP(hipStreamSynchronize(s));
    B_HIP(hipEventRecord(b->ev0, s));
    for (uint32_t i = 0; i < iters; i++) {
        rc = jpgpu_batch_decode(b, hip_stream);
        if (rc) return rc;
    }
    B_HIP(hipEventRecord(b->ev1, s));
    B_HIP(hipEventSynchronize(b->ev1));
    float ms = 0.f;
    B_HIP(hipEventElapsedTime(&ms, b->ev0, b->ev1));
    *ms_per_decode = ms / (float)iters;
    return JPGPU_OK;
}

}  // extern "C"
