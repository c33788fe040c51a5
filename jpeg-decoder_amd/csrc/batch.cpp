// batch.cpp — batch driver of the C ABI (include/jpgpu.h, jpgpu_batch_*).
//
// A batch is N independent images (the unit the reference decodes one-per-Decoder,
// src/decoder.rs:134-154) laid out in two HBM arenas: all coefficient planes (int16,
// block-raster = the concatenation of each component's append_row buffers)
// and all output pixels.  One decode = a handful of launches over the whole batch.
// Images of a fusable kind (4:2:0 YCbCr, 4:4:4 YCbCr / RGB, gray; any size) are grouped per kind and run the fused
// kernels (fused.hip), one launch group per kind; everything else runs the generic two-kernel path (kernels.hip)
// through device job tables.  jpgpu_batch_path names the kernels: "fused420", ..., "generic", or "mixed".  (An output size: batch_output.cpp.)
#include "batch_internal.hpp"

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

static int batch_refresh_jobs(jpgpu_batch *b, hipStream_t stream = nullptr) {
    // host-side classes are part of the launch tables (one launch per class: fused_bind); with device-side classes they
    // travel in a small table of their own, asynchronously, and the launch tables stay as they are
    const bool need_bind = b->jobs_dirty || (b->cls_dirty && !b->dev_classes);
    if (!need_bind && b->d_coef && b->d_out) {  // (other flips or matrices alone: the records that hold them, nothing else)
        int rc = output_bind(b, stream, false);
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
    rc = output_bind(b, stream, true);
    if (rc) return rc;
    if (b->qt_dirty) {
        rc = batch_upload_qt(b);
        if (rc) return rc;
        b->qt_dirty = false;
    }
    b->jobs_dirty = false;
    return JPGPU_OK;
}

extern "C" {

// placements: those of jpgpu_batch_create_placed (NULL, or without an output size: none); orientations: those of
// jpgpu_batch_create_oriented (NULL: none) — the windows are then windows of the oriented images; spec_: everything else of the
// fixed-output stage
static int batch_create(int device, const jpgpu_image_desc *descs, const jpgpu_window *windows, const jpgpu_placement *placements, uint32_t n_images,
                        uint32_t flags, const OutputSpec &spec_, jpgpu_batch **out, const uint8_t *orientations = nullptr) {
    if (!out) return JPGPU_ERR_FORMAT;
    *out = nullptr;
    if (!descs || n_images == 0 || n_images > 65535) return JPGPU_ERR_FORMAT;
    jpgpu_batch *b = new jpgpu_batch();
    *out = b;  // returned even on failure so the caller can read last_error, then destroy
    b->device = device;
    b->flags = flags;
    OutputSpec spec = spec_;
    const uint32_t bad = check_orientations(orientations, n_images, spec.orient);  // (all ones is none: the batch without the argument)
    if (bad < n_images) return set_err(b->err, JPGPU_ERR_FORMAT, "image %u: orientation %u (the values are 1..8)", bad, orientations[bad]);
    b->o.spec = spec;
    if (spec.orient) b->o.orient.assign(orientations, orientations + n_images);
    const bool resized = spec.sized();
    std::string why;
    int rc = output_rule(spec, why);
    if (rc) return set_err(b->err, rc, "%s", why.c_str());
    for (uint32_t i = 0; i < n_images; i++)  // (the format against the channels of every image of the call, before a device is touched)
        if (output_tensor_rule(spec, std::min<uint32_t>(std::max<uint32_t>(descs[i].ncomp, 1u), 4u), why)) return set_err(b->err, JPGPU_ERR_FORMAT, "image %u: %s", i, why.c_str());
    if (placements && resized) {  // (every placement shows a pixel; one that differs from the whole output makes the batch a placed one)
        const uint32_t i = normalise_placements(placements, n_images, spec.w, spec.h, b->o.pl, b->o.placed);
        if (i < n_images)
            return set_err(b->err, JPGPU_ERR_FORMAT, "image %u: the placement %ux%u at (%d, %d) shows no pixel of the %ux%u output", i, b->o.pl[i].rw, b->o.pl[i].rh,
                           b->o.pl[i].x, b->o.pl[i].y, spec.w, spec.h);
    }
    rc = use_device(device, b->err);
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
        rc = output_image_rule(spec, d.ncomp, ij.color_fn, why);
        if (rc) return set_err(b->err, rc, "image %u: %s", i, why.c_str());
        // a window smaller than the image: the window group (an empty window or one that covers the image is no window)
        bool windowed = false;
        if (windows) {
            uint32_t gw = 0, gh = 0;
            WindowGeom wg;
            jpgpu_window wn = windows[i];
            if (spec.orient) rc = orient_window_rule(d, orientations[i], wn, why);  // (the source window: what the routes below decode)
            if (rc) return set_err(b->err, rc, "image %u: %s", i, why.c_str());
            rc = window_rule(d, wn, windowed, gw, gh, wg, why);
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
    if (spec.orient) b->path += "+orient";
    if (spec.rgb) b->path += "+rgb";
    if (b->o.placed) b->path += "+place";
    if (resized) b->path += "+resize";
    if (spec.filter) b->path += std::string(":") + resample_filter_name(spec.filter);
    if (spec.colour) b->path += "+colour";
    if (spec.warp) b->path += spec.wp.filter == WP_BILINEAR ? "+warp:bilinear" : "+warp";
    if (spec.tensor) b->path += "+tensor";
    rc = output_create(b);  // (what was laid out so far becomes the intermediate arena)
    if (rc) return rc;
    const size_t full = arena_layout(b->out_full_len);  // (what the whole images take)
    if (!(flags & JPGPU_BATCH_EXTERNAL_BUFFERS)) {
        B_HIP(hipMalloc((void **)&b->d_coef, b->coef_bytes));
        b->own_coef = true;
        // (with windows: a quarter more than these need, at most what the whole images take — batch_rewindow sets other windows in place)
        b->out_cap = (b->win.empty() || resized) ? b->out_bytes : arena_headroom(b->out_bytes, full);
        B_HIP(hipMalloc((void **)&b->d_out, b->out_cap));
        b->own_out = true;
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
    return resized ? output_retable(b) : JPGPU_OK;
}

// The spec of a public creator: the size, the RGB and filter bits of its flags, and the options it has (NULL: none).
static OutputSpec spec_of(uint32_t flags, uint32_t w = 0, uint32_t h = 0, const jpgpu_tensor_format *tensor = nullptr, const uint8_t *fill = nullptr,
                          const jpgpu_warp_options *warp = nullptr) {
    OutputSpec s;
    s.w = w, s.h = h, s.rgb = (flags & JPGPU_BATCH_RGB_OUTPUT) != 0;
    s.filter = (flags >> 8) & 15u;  // JPGPU_BATCH_FILTER(f): 0 is BILINEAR, so flags without the bits mean what they meant
    if (tensor) s.tensor = true, s.tn = *tensor;
    if (fill) memcpy(s.fill, fill, 4);
    if (warp) s.warp = true, s.wp = *warp;
    return s;
}
// A creator with an output size was given none (0 x 0 would mean "none" to batch_create): a batch that holds the creator's own message.
static int refuse_no_size(jpgpu_batch **out, const char *message, uint32_t w, uint32_t h) {
    if (!out) return JPGPU_ERR_FORMAT;
    *out = new jpgpu_batch();
    return set_err((*out)->err, JPGPU_ERR_FORMAT, message, w, h, RS_MAX_OUT);
}
static const char kNoSize[] = "output size %ux%u: width and height must be 1..%u";

int jpgpu_batch_create(int device, const jpgpu_image_desc *descs, uint32_t n_images, uint32_t flags, jpgpu_batch **out) {
    return batch_create(device, descs, nullptr, nullptr, n_images, flags, spec_of(flags), out);
}
int jpgpu_batch_create_windowed(int device, const jpgpu_image_desc *descs, const jpgpu_window *windows, uint32_t n_images, uint32_t flags, jpgpu_batch **out) {
    return batch_create(device, descs, windows, nullptr, n_images, flags, spec_of(flags), out);
}
int jpgpu_batch_create_resized(int device, const jpgpu_image_desc *descs, const jpgpu_window *windows, uint16_t out_w, uint16_t out_h, uint32_t n_images, uint32_t flags,
                               jpgpu_batch **out) {
    if (out_w == 0 || out_h == 0) return refuse_no_size(out, kNoSize, out_w, out_h);
    return batch_create(device, descs, windows, nullptr, n_images, flags, spec_of(flags, out_w, out_h), out);
}
int jpgpu_batch_create_tensor(int device, const jpgpu_image_desc *descs, const jpgpu_window *windows, uint16_t out_w, uint16_t out_h,
                              const jpgpu_tensor_format *format, uint32_t n_images, uint32_t flags, jpgpu_batch **out) {
    if (out_w == 0 || out_h == 0 || !format)  // (no output size, no format: below they would mean "none")
        return refuse_no_size(out, format ? "a tensor format needs an output size (%ux%u: width and height must be 1..%u)" : "jpgpu_batch_create_tensor: no tensor format", out_w, out_h);
    return batch_create(device, descs, windows, nullptr, n_images, flags, spec_of(flags, out_w, out_h, format), out);
}
int jpgpu_batch_create_placed(int device, const jpgpu_image_desc *descs, const jpgpu_window *windows, const jpgpu_placement *placements, const uint8_t *fill,
                              uint16_t out_w, uint16_t out_h, const jpgpu_tensor_format *format, uint32_t n_images, uint32_t flags, jpgpu_batch **out) {
    return jpgpu_batch_create_warped(device, descs, windows, placements, fill, out_w, out_h, format, nullptr, n_images, flags, out);
}
int jpgpu_batch_create_warped(int device, const jpgpu_image_desc *descs, const jpgpu_window *windows, const jpgpu_placement *placements, const uint8_t *fill,
                              uint16_t out_w, uint16_t out_h, const jpgpu_tensor_format *format, const jpgpu_warp_options *warp, uint32_t n_images, uint32_t flags,
                              jpgpu_batch **out) {
    return jpgpu_batch_create_oriented(device, descs, windows, placements, fill, out_w, out_h, format, warp, nullptr, n_images, flags, out);
}
int jpgpu_batch_create_oriented(int device, const jpgpu_image_desc *descs, const jpgpu_window *windows, const jpgpu_placement *placements, const uint8_t *fill,
                                uint16_t out_w, uint16_t out_h, const jpgpu_tensor_format *format, const jpgpu_warp_options *warp, const uint8_t *orientations,
                                uint32_t n_images, uint32_t flags, jpgpu_batch **out) {
    if (out_w == 0 || out_h == 0) {
        bool any = false;
        const bool valid = check_orientations(orientations, n_images, any) == n_images;
        if (out && valid && any) {  // (orientations without an output size: the rule's own refusal, as RGB output)
            std::string why;
            OutputSpec s;
            s.orient = true;
            *out = new jpgpu_batch();
            return set_err((*out)->err, output_rule(s, why), "%s", why.c_str());
        }
        return refuse_no_size(out, !valid ? "an orientation outside 1..8 (output size %ux%u: width and height must be 1..%u)"
                                   : warp ? "a warp needs an output size (%ux%u: width and height must be 1..%u)" : kNoSize, out_w, out_h);
    }
    return batch_create(device, descs, windows, placements, n_images, flags, spec_of(flags, out_w, out_h, format, fill, warp), out, orientations);
}
int jpgpu_batch_create_coloured(int device, const jpgpu_image_desc *descs, const jpgpu_window *windows, const jpgpu_placement *placements, const uint8_t *fill,
                                uint16_t out_w, uint16_t out_h, const jpgpu_tensor_format *format, const jpgpu_warp_options *warp, const uint8_t *orientations,
                                const jpgpu_colour_options *colour, uint32_t n_images, uint32_t flags, jpgpu_batch **out) {
    if (!colour) return jpgpu_batch_create_oriented(device, descs, windows, placements, fill, out_w, out_h, format, warp, orientations, n_images, flags, out);
    if (!out) return JPGPU_ERR_FORMAT;
    if (colour->reserved != 0u) return *out = new jpgpu_batch(), set_err((*out)->err, JPGPU_ERR_FORMAT, "colour options: reserved %u (must be 0)", colour->reserved);
    OutputSpec s = spec_of(flags, out_w, out_h, format, fill, warp);
    s.colour = true;
    if (out_w == 0 || out_h == 0) {  // (colour without an output size: the rule's own refusal, as RGB output)
        std::string why;
        OutputSpec none;
        none.colour = true;
        *out = new jpgpu_batch();
        return set_err((*out)->err, output_rule(none, why), "%s", why.c_str());
    }
    return batch_create(device, descs, windows, placements, n_images, flags, s, out, orientations);
}
void jpgpu_batch_destroy(jpgpu_batch *b) {
    if (!b) return;
    std::string err;
    if (use_device(b->device, err) == JPGPU_OK) {
        hipDeviceSynchronize();
        if (b->own_coef && b->d_coef) hipFree(b->d_coef);
        if (b->own_out && b->d_out) hipFree(b->d_out);
        for (void *d : {(void *)b->d_planes, (void *)b->d_qt, (void *)b->d_compact, (void *)b->d_expand_jobs, (void *)b->d_entropy, (void *)b->d_scan, (void *)b->d_stats,
                        (void *)b->d_host_cls, (void *)b->d_plane_job_slot, (void *)b->d_plane_jobs, (void *)b->d_image_jobs})
            if (d) hipFree(d);
        for (void *h : {(void *)b->h_expand_jobs, (void *)b->h_entropy, (void *)b->h_entropy_out, (void *)b->h_bounce, (void *)b->h_scan, (void *)b->h_host_cls})
            if (h) hipHostFree(h);
        for (hipEvent_t e : {b->expand_sent, b->entropy_uploaded, b->entropy_filled, b->ev0, b->ev1, b->enqueued})
            if (e) hipEventDestroy(e);
        for (auto &e : b->cls_sent)
            if (e) hipEventDestroy(e);
        for (auto &e : b->ev_phase)
            if (e) hipEventDestroy(e);
        b->o.free();
        b->scaled.free();
        b->win.free();
        for (FusedPlan &fp : b->fused) fused_free(fp);
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

int jpgpu::batch_create_with(int device, const jpgpu_image_desc *descs, const jpgpu_window *windows, const jpgpu_placement *placements, uint32_t n_images,
                             const OutputSpec &spec, jpgpu_batch **out, const uint8_t *orientations) {
    return batch_create(device, descs, windows, placements, n_images, JPGPU_BATCH_DEFAULT, spec, out, orientations);
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
    OutputStage &o = b->o;
    const bool sized = o.spec.sized();
    if ((!b->own_out && !sized) || b->win.empty()) return JPGPU_ERR_UNSUPPORTED;  // (with an output size the windows' bytes are the batch's own)
    std::vector<jpgpu_placement> pls;
    if (placements) {
        bool any = false;
        if (normalise_placements(placements, (uint32_t)b->descs.size(), o.spec.w, o.spec.h, pls, any) < b->descs.size()) return JPGPU_ERR_FORMAT;
        if (any != o.placed) return JPGPU_ERR_UNSUPPORTED;
    }
    std::vector<WindowGeom> geoms;
    std::vector<size_t> lens;
    std::vector<jpgpu_window> source;
    if (o.route.orient) {  // (windows of the oriented images: the source windows, as at creation)
        source.assign(windows, windows + b->descs.size());
        std::string why;
        for (size_t i = 0; i < source.size(); i++)
            if (orient_window_rule(b->descs[i], o.orient[i], source[i], why)) return JPGPU_ERR_UNSUPPORTED;
        windows = source.data();
    }
    int rc = window_rule_rewindow(b->descs, b->win.ids, b->out_full_len, windows, geoms, lens);
    if (rc) return rc;
    rc = use_device(b->device, b->err);
    if (rc) return rc;
    // (with an output size the windows' bytes live in the intermediate arena: the resized arena never changes)
    size_t &w_bytes = sized ? o.pix_bytes : b->out_bytes, &w_cap = sized ? o.pix_cap : b->out_cap;
    uint8_t *&w_arena = sized ? o.d_pix : b->d_out;
    w_bytes = sized ? arena_layout(lens, o.pix_off, o.pix_len) : arena_layout(lens, b->out_off, b->out_len);
    b->jobs_dirty = true;  // (every job's output pointer, the fused plans' included)
    B_HIP(batch_wait_enqueued(b));  // (idle by contract: the event has completed)
    if (w_bytes > w_cap) {
        B_HIP(hipDeviceSynchronize());
        B_HIP(grow_device(w_arena, w_cap, w_bytes, arena_headroom(w_bytes, arena_layout(b->out_full_len))));
    }
    B_HIP(b->win.set_geoms(geoms, b->descs));
    if (o.placed && placements) o.pl = pls;
    return sized ? output_retable(b) : JPGPU_OK;
}
// bytes the output arena of the batch would hold without any window (what a pinned copy of it never needs more than)
size_t jpgpu::batch_out_arena_bound(const jpgpu_batch *b) {
    if (b && b->o.spec.sized()) return b->out_bytes;  // (an output size: the arena never changes)
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
    rc = output_launch(b, s);  // (an output size: the resample and what follows it)
    if (rc) return rc;
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
