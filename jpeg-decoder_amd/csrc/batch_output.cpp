// batch_output.cpp — the fixed-output stage of a batch (jpgpu_batch::o, batch_internal.hpp): its arenas and tables at creation, its
// job records on a refresh, its launches behind the pixel kernels of a decode.  The options, the rules and the route: batch_output.hpp.
#include <array>
#include <map>

#include "batch_internal.hpp"
#include "colour_pixel_band.hpp"

static const jpgpu_warp kIdentity{{1.0, 0.0, 0.0, 0.0, 1.0, 0.0}};
// JPGPU_CL_STRIP_ROWS, read per call: the rows of a SHARPNESS strip (clamped by cl_strip_rows to what LDS holds); unset or 0: as many
// as LDS holds.  The tests reach strip seams on small images with it.
static uint32_t colour_strip_rows_knob() {
    const char *knob = getenv("JPGPU_CL_STRIP_ROWS");
    const int v = knob ? atoi(knob) : 0;
    return v > 0 ? (uint32_t)v : 0u;
}
static size_t warp_jobs_bytes(const jpgpu_batch *b) { return b->descs.size() * (sizeof(WarpJob) + ((size_t)b->o.spec.w + b->o.spec.h) * sizeof(int32_t)); }

// At creation, once the intermediate arena is laid out as the output arena (out_off, out_len, out_bytes): that layout becomes the
// intermediate arena's, the output arena holds the spec's bytes per image, and the stage's device blocks are allocated by the route.
int output_create(jpgpu_batch *b) {
    OutputStage &o = b->o;
    const uint32_t n = (uint32_t)b->descs.size();
    if (!o.spec.sized()) return JPGPU_OK;
    o.route = output_route(o.spec, o.placed, 0u);
    o.pix_off = b->out_off, o.pix_len = b->out_len, o.pix_bytes = b->out_bytes;
    b->out_bytes = output_arena(o.spec, b->descs, false, b->out_off, b->out_len);
    // (the same headroom for other windows as the output arena of a batch without an output size has)
    o.pix_cap = b->win.empty() ? o.pix_bytes : arena_headroom(o.pix_bytes, arena_layout(b->out_full_len));
    B_HIP(hipMalloc((void **)&o.d_pix, o.pix_cap));
    if (o.spec.tensor) o.flips.assign(n, 0);
    if (o.route.warp) {  // (every image starts with the identity)
        std::vector<size_t> wsrc_len;
        o.m.assign(n, kIdentity);
        B_HIP(hipMalloc((void **)&o.d_wsrc, output_arena(o.spec, b->descs, true, o.wsrc_off, wsrc_len)));
        B_HIP(hipMalloc((void **)&o.d_wp_jobs, warp_jobs_bytes(b)));
        o.wp_dirty = true;
    }
    if (o.route.colour) {  // (every image starts with the empty program)
        double scale[256];
        colour_scale_table(scale);
        o.programs.assign(n, ColourProgram{});
        B_HIP(hipMalloc((void **)&o.d_cl_jobs, (size_t)n * sizeof(ColourJob)));
        B_HIP(hipMalloc((void **)&o.d_cl_scale, sizeof scale));
        B_HIP(hipMemcpy(o.d_cl_scale, scale, sizeof scale, hipMemcpyHostToDevice));
        o.cl_dirty = true;
    }
    if (o.spec.tensor) {  // (the table of four channels: every image looks up its own first ncomp rows)
        B_HIP(hipMalloc(&o.d_tn_table, TN_TABLE_MAX));
        std::vector<uint32_t> table(TN_TABLE_MAX / 4u, 0u);
        uint32_t nc_max = 1u;
        for (const jpgpu_image_desc &d : b->descs) nc_max = std::max(nc_max, o.spec.channels(d.ncomp));
        tensor_table(o.spec.tn.dtype, o.spec.tn.mean, o.spec.tn.std, nc_max, table.data());
        B_HIP(hipMemcpy(o.d_tn_table, table.data(), TN_TABLE_MAX, hipMemcpyHostToDevice));
    }
    const size_t record = o.route.resample == Resample::PlacedTensor ? sizeof(PlacedTensorJob) : o.route.resample == Resample::Tensor ? 2u * sizeof(TensorJob)
                          : o.route.resample == Resample::Placed     ? sizeof(PlacedJob) : 2u * sizeof(ResampleJob);
    B_HIP(hipMalloc(&o.d_jobs, (size_t)n * record));
    if (!o.placed) B_HIP(hipMalloc((void **)&o.d_bpr, (size_t)n * sizeof(uint32_t)));
    if (o.route.orient) {  // (the jobs of the images with another orientation than 1; output_retable lays their arena out)
        for (uint32_t i = 0; i < n; i++)
            if (o.orient[i] != 1u) o.or_ids.push_back(i);
        B_HIP(hipMalloc((void **)&o.d_or_jobs, o.or_ids.size() * sizeof(OrientJob)));
    }
    return JPGPU_OK;
}

// The orientation jobs and their arena from the source sizes in o.jobs (the windows', else the output grids'), and the oriented sizes
// into o.jobs: the resample of an oriented image reads the oriented window.
static int orient_retable(jpgpu_batch *b) {
    OutputStage &o = b->o;
    o.or_off.assign(b->descs.size(), 0);
    o.or_jobs.assign(o.or_ids.size(), OrientJob{});
    o.or_max_tiles = 0;
    size_t bytes = 0;
    for (size_t k = 0; k < o.or_ids.size(); k++) {
        const uint32_t i = o.or_ids[k];
        ResampleJob &j = o.jobs[i];
        OrientJob &oj = o.or_jobs[k];
        oj.w = j.in_w, oj.h = j.in_h, oj.nc = b->descs[i].ncomp, oj.o = o.orient[i];
        orient_job_tiles(oj);
        o.or_max_tiles = std::max(o.or_max_tiles, oj.tiles);
        oriented_size(oj.o, oj.w, oj.h, j.in_w, j.in_h);
        o.or_off[i] = bytes;
        bytes += align_up(orient_bytes(oj.w, oj.h, oj.nc), 256);
    }
    if (bytes > o.or_cap) {
        B_HIP(batch_wait_enqueued(b));  // (a decode still queued writes the arena)
        B_HIP(hipDeviceSynchronize());
        B_HIP(grow_device(o.d_or, o.or_cap, bytes, b->win.empty() ? bytes : quarter_more(bytes)));
    }
    return JPGPU_OK;
}

// The resample tables and bands of every image from its source size (its window's, else its output grid's): at creation and after
// batch_rewindow.  Axes of equal (in, out) sizes share one table.
int output_retable(jpgpu_batch *b) {
    OutputStage &o = b->o;
    const uint32_t n = (uint32_t)b->descs.size();
    o.jobs.assign(n, ResampleJob{});
    o.tab.clear();
    o.max_bands = o.lds_bytes = o.max_runs = 0;
    o.bpr.assign(n, 0u);
    const uint32_t filter = o.spec.filter;  // (one per batch: the keys need not hold it)
    // entries [first, first + count) of the axis (in, out) -> offsets of bounds, coefficients.  A placed batch tabulates the visible
    // range and nothing else; the others the whole axis.
    std::map<std::array<uint32_t, 4>, std::pair<uint32_t, uint32_t>> seen;
    auto axis = [&](uint32_t in, uint32_t out, uint32_t first, uint32_t count, uint32_t &bo, uint32_t &ko, uint32_t &ks) {
        ks = resample_ksize_filtered(filter, in, out);
        const std::array<uint32_t, 4> key = {in, out, first, count};
        auto it = seen.find(key);
        if (it != seen.end()) return bo = it->second.first, ko = it->second.second, true;
        const size_t base = o.tab.size(), end = base + 2u * (size_t)count + (size_t)count * ks;
        if (end > 0xffffffffull) return false;
        o.tab.resize(end);
        bo = (uint32_t)base, ko = (uint32_t)(base + 2u * count);
        if (o.placed) resample_coefficients_range_filtered(filter, in, out, first, count, o.tab.data() + bo, o.tab.data() + ko, ks);
        else resample_coefficients_filtered(filter, in, out, o.tab.data() + bo, o.tab.data() + ko, ks);
        seen[key] = {bo, ko};
        return true;
    };
    if (o.placed) o.places.assign(n, Place{});
    size_t k = 0;
    for (uint32_t i = 0; i < n; i++) {
        const jpgpu_image_desc &d = b->descs[i];
        ResampleJob &j = o.jobs[i];
        window_grid(d.components, d.ncomp, d.out_w, d.out_h, j.in_w, j.in_h);
        if (k < b->win.ids.size() && b->win.ids[k] == i) j.in_w = b->win.geoms[k].ww, j.in_h = b->win.geoms[k].wh, k++;
    }
    if (o.route.orient) {
        const int rc = orient_retable(b);
        if (rc) return rc;
    }
    for (uint32_t i = 0; i < n; i++) {
        const jpgpu_image_desc &d = b->descs[i];
        ResampleJob &j = o.jobs[i];
        j.nc = d.ncomp, j.out_w = o.spec.w, j.out_h = o.spec.h;
        if (o.spec.rgb) j.nc = 3u, j.src_nc = d.ncomp == 3u ? 0u : d.ncomp;  // (gray / CMYK: converted by the horizontal pass)
        jpgpu_placement pl{(uint16_t)o.spec.w, (uint16_t)o.spec.h, 0, 0};
        uint32_t fx = 0, fy = 0;
        if (o.placed) {  // (the job of the visible rectangle)
            pl = o.pl[i];
            Place &p = o.places[i];
            if (!placed_axis(pl.rw, pl.x, o.spec.w, fx, j.out_w, p.vx) || !placed_axis(pl.rh, pl.y, o.spec.h, fy, j.out_h, p.vy))
                return set_err(b->err, JPGPU_ERR_FORMAT, "image %u: the placement shows no pixel", i);
            p.cw = o.spec.w, p.ch = o.spec.h, p.fill = pack_fill(o.spec.fill);
        }
        if (!axis(j.in_w, pl.rw, fx, j.out_w, j.hb, j.hk, j.hks) || !axis(j.in_h, pl.rh, fy, j.out_h, j.vb, j.vk, j.vks))
            return set_err(b->err, JPGPU_ERR_UNSUPPORTED, "image %u: resample tables of the batch exceed 2^32 words", i);
    }
    for (uint32_t i = 0; i < n; i++) {  // (the tables stand still now)
        ResampleJob &j = o.jobs[i];
        if (o.placed) {
            if (!placed_plan(j, o.places[i], o.tab.data())) return set_err(b->err, JPGPU_ERR_INTERNAL, "image %u: no resample plan", i);
            o.max_bands = std::max(o.max_bands, o.places[i].bands);
        } else {
            if (!resample_plan(j, o.tab.data())) return set_err(b->err, JPGPU_ERR_INTERNAL, "image %u: no resample plan", i);
            // (JPGPU_RS_ROLL, read per call: 1 never, 2 / 4 / 8 every candidate with that many bands per run — the benchmark's A/B)
            const char *knob = getenv("JPGPU_RS_ROLL");
            const uint32_t bpr = o.bpr[i] = resample_roll_bpr(j, o.tab.data(), filter, knob ? (uint32_t)atoi(knob) : 0u);
            if (bpr) o.max_runs = std::max(o.max_runs, (j.bands + bpr - 1u) / bpr);
            else o.max_bands = std::max(o.max_bands, j.bands);
        }
        o.lds_bytes = std::max(o.lds_bytes, j.lds_bytes);
    }
    o.route = output_route(o.spec, o.placed, o.max_runs);
    const size_t roll_at = b->path.find("+roll");  // (the path names the route where any image took it; other windows may change that)
    if (roll_at != std::string::npos) b->path.erase(roll_at, 5);
    // (the last word of the u8 batch's path: in front of the colour's and the warp's)
    if (o.route.runs) b->path.insert(std::min(std::min(b->path.find("+colour"), b->path.find("+warp")), b->path.size()), "+roll");
    B_HIP(batch_wait_enqueued(b));  // (a decode still queued reads the tables)
    if (o.tab.size() > o.tab_cap) {
        B_HIP(hipDeviceSynchronize());
        B_HIP(grow_device(o.d_tab, o.tab_cap, o.tab.size()));
    }
    B_HIP(hipMemcpy(o.d_tab, o.tab.data(), o.tab.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (o.d_bpr) B_HIP(hipMemcpy(o.d_bpr, o.bpr.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    b->jobs_dirty = true;  // (the jobs go up with the others)
    return JPGPU_OK;
}

// The records of a tensor route: every image's resample job, its plane pitch and its flip (placed: its placement behind them).  They
// travel on the decode's stream from the pinned mirror (a blocking copy per sub-batch would hold a loader's uploader thread up).
static int upload_tensor_jobs(jpgpu_batch *b, hipStream_t stream) {
    OutputStage &o = b->o;
    const uint32_t n = (uint32_t)b->descs.size();
    const bool placed = o.route.resample == Resample::PlacedTensor;
    const size_t bytes = (size_t)n * (placed ? sizeof(PlacedTensorJob) : (o.route.runs ? 2u : 1u) * sizeof(TensorJob));
    if (!o.h_jobs) {
        B_HIP(hipHostMalloc(&o.h_jobs, (size_t)n * (placed ? sizeof(PlacedTensorJob) : 2u * sizeof(TensorJob)), hipHostMallocDefault));
        B_HIP(hipEventCreateWithFlags(&o.tn_sent, hipEventDisableTiming));
    } else {
        B_HIP(hipEventSynchronize(o.tn_sent));  // (the copy before this one has read the mirror)
    }
    for (uint32_t i = 0; i < n; i++) {
        TensorJob t;
        t.r = o.jobs[i], t.plane = o.spec.w * o.spec.h, t.flip = o.flips[i] ? 1u : 0u;
        if (placed) {
            static_cast<PlacedTensorJob *>(o.h_jobs)[i] = PlacedTensorJob{t, o.places[i]};
            continue;
        }
        TensorJob *h = static_cast<TensorJob *>(o.h_jobs);
        h[i] = t;
        if (!o.route.runs) continue;
        h[n + i] = t;                       // (the run launch's: the real job)
        if (o.bpr[i]) h[i].r.bands = 0u;  // (the band launch's: no band of this image)
    }
    B_HIP(hipMemcpyAsync(o.d_jobs, o.h_jobs, bytes, hipMemcpyHostToDevice, stream));
    B_HIP(hipEventRecord(o.tn_sent, stream));
    o.tn_dirty = false;
    return JPGPU_OK;
}

// The WarpJobs of a warped batch and the N-sep tables behind them: every image's matrix, its flip, where it reads and writes.  From a
// pinned mirror on the decode's stream, as the tensor records: a decode queued earlier keeps the matrices it was enqueued with.
static int upload_warp_jobs(jpgpu_batch *b, hipStream_t stream) {
    OutputStage &o = b->o;
    const uint32_t n = (uint32_t)b->descs.size();
    if (!o.h_wp_jobs) {
        B_HIP(hipHostMalloc((void **)&o.h_wp_jobs, warp_jobs_bytes(b), hipHostMallocDefault));
        B_HIP(hipEventCreateWithFlags(&o.wp_sent, hipEventDisableTiming));
    } else {
        B_HIP(hipEventSynchronize(o.wp_sent));  // (the copy before this one has read the mirror)
    }
    WarpJob *jobs = reinterpret_cast<WarpJob *>(o.h_wp_jobs);
    int32_t *tabs = reinterpret_cast<int32_t *>(o.h_wp_jobs + (size_t)n * sizeof(WarpJob));
    for (uint32_t i = 0; i < n; i++) {
        WarpJob &j = jobs[i];
        j.src = o.d_wsrc + o.wsrc_off[i], j.dst = b->d_out + b->out_off[i];
        j.w = o.spec.w, j.h = o.spec.h, j.nc = o.spec.channels(b->descs[i].ncomp);
        j.flip = (o.spec.tensor && o.flips[i]) ? 1u : 0u;
        j.fill = pack_fill(o.spec.wp.fill), j.plane = o.spec.w * o.spec.h;
        j.tab = i * (o.spec.w + o.spec.h);
        warp_job_matrix(j, o.m[i].m, o.spec.wp.filter, tabs + j.tab);
    }
    B_HIP(hipMemcpyAsync(o.d_wp_jobs, o.h_wp_jobs, warp_jobs_bytes(b), hipMemcpyHostToDevice, stream));
    B_HIP(hipEventRecord(o.wp_sent, stream));
    o.wp_dirty = false;
    return JPGPU_OK;
}

// The ColourJobs of a coloured batch: every image's program and where the u8 resample left its pixels.  From a pinned mirror on the
// decode's stream, as the WarpJobs: a decode queued earlier keeps the programs it was enqueued with.
static int upload_colour_jobs(jpgpu_batch *b, hipStream_t stream) {
    OutputStage &o = b->o;
    const uint32_t n = (uint32_t)b->descs.size();
    if (!o.h_cl_jobs) {
        B_HIP(hipHostMalloc((void **)&o.h_cl_jobs, (size_t)n * sizeof(ColourJob), hipHostMallocDefault));
        B_HIP(hipEventCreateWithFlags(&o.cl_sent, hipEventDisableTiming));
    } else {
        B_HIP(hipEventSynchronize(o.cl_sent));  // (the copy before this one has read the mirror)
    }
    for (uint32_t i = 0; i < n; i++) colour_job(o.h_cl_jobs[i], o.d_wsrc + o.wsrc_off[i], o.spec.w, o.spec.h, &o.programs[i]);
    B_HIP(hipMemcpyAsync(o.d_cl_jobs, o.h_cl_jobs, (size_t)n * sizeof(ColourJob), hipMemcpyHostToDevice, stream));
    B_HIP(hipEventRecord(o.cl_sent, stream));
    o.cl_dirty = false;
    return JPGPU_OK;
}

// On a refresh of the job tables (batch_refresh_jobs).  `all` false — nothing else is rebound: the records whose flips or matrices
// changed, alone.  `all`: every record, with where the images lie in the arenas now; the blocking copies follow the caller's wait.
int output_bind(jpgpu_batch *b, hipStream_t stream, bool all) {
    OutputStage &o = b->o;
    const uint32_t n = (uint32_t)b->descs.size();
    int rc = JPGPU_OK;
    if (!all) {
        if (o.tn_dirty) rc = upload_tensor_jobs(b, stream);
        if (rc == JPGPU_OK && o.wp_dirty) rc = upload_warp_jobs(b, stream);
        if (rc == JPGPU_OK && o.cl_dirty) rc = upload_colour_jobs(b, stream);
        return rc;
    }
    if (o.route.resample == Resample::None) return JPGPU_OK;
    for (uint32_t i = 0; i < n; i++) o.jobs[i].src = o.d_pix + o.pix_off[i], o.jobs[i].dst = o.route.warp ? o.d_wsrc + o.wsrc_off[i] : b->d_out + b->out_off[i];
    if (o.route.orient) {  // (an oriented image: out of the intermediate arena into the oriented one, where its resample reads)
        for (size_t k = 0; k < o.or_ids.size(); k++) {
            const uint32_t i = o.or_ids[k];
            o.or_jobs[k].src = o.d_pix + o.pix_off[i], o.or_jobs[k].dst = o.d_or + o.or_off[i];
            o.jobs[i].src = o.or_jobs[k].dst;
        }
        B_HIP(hipMemcpy(o.d_or_jobs, o.or_jobs.data(), o.or_jobs.size() * sizeof(OrientJob), hipMemcpyHostToDevice));
    }
    if (o.route.warp) rc = upload_warp_jobs(b, stream);  // (the u8 resample of the same arguments writes the warp's source; the warp writes the output)
    if (rc == JPGPU_OK && o.route.colour) rc = upload_colour_jobs(b, stream);  // (in place on the warp's source, between the two)
    if (rc) return rc;
    if (o.route.tensor_jobs()) return upload_tensor_jobs(b, stream);
    if (o.route.resample == Resample::Placed) {
        std::vector<PlacedJob> pj(n);
        for (uint32_t i = 0; i < n; i++) pj[i].r = o.jobs[i], pj[i].p = o.places[i];
        B_HIP(hipMemcpy(o.d_jobs, pj.data(), (size_t)n * sizeof(PlacedJob), hipMemcpyHostToDevice));
    } else {  // (band launch: images in runs have no band; run launch, behind them: the real jobs)
        std::vector<ResampleJob> both(o.jobs);
        if (o.route.runs) both.insert(both.end(), o.jobs.begin(), o.jobs.end());
        for (uint32_t i = 0; o.route.runs && i < n; i++)
            if (o.bpr[i]) both[i].bands = 0u;
        B_HIP(hipMemcpy(o.d_jobs, both.data(), both.size() * sizeof(ResampleJob), hipMemcpyHostToDevice));
    }
    return JPGPU_OK;
}

// On a decode, behind the pixel kernels on `s`: the orientation launch, the route's resample launch, the launch of runs beside it, the
// colour launch and the warp behind them.
int output_launch(jpgpu_batch *b, hipStream_t s) {
    const OutputStage &o = b->o;
    const uint32_t n = (uint32_t)b->descs.size(), es = o.spec.elem_bytes();
    if (o.spec.tensor && o.tn_sent) B_HIP(hipStreamWaitEvent(s, o.tn_sent, 0));  // (the jobs may have gone up on another stream than this one)
    if (o.route.orient) B_HIP(launch_orient(o.d_or_jobs, (uint32_t)o.or_jobs.size(), o.or_max_tiles, s));  // (in front of the resample: it reads the oriented arena)
    // (placements: the kernels of placed.hip; a tensor output: the same resample, its vertical pass writes every image's tensor; else
    // every image's pixels — wherever the launches before left them in the intermediate arena)
    switch (o.route.resample) {
    case Resample::None: break;
    case Resample::PlacedTensor: B_HIP(launch_resample_placed_tensor(static_cast<const PlacedTensorJob *>(o.d_jobs), o.d_tab, o.d_tn_table, es, n, o.max_bands, o.lds_bytes, s, o.spec.rgb)); break;
    case Resample::Placed: B_HIP(launch_resample_placed(static_cast<const PlacedJob *>(o.d_jobs), o.d_tab, n, o.max_bands, o.lds_bytes, s, o.spec.rgb)); break;
    case Resample::Tensor: B_HIP(launch_resample_tensor(static_cast<const TensorJob *>(o.d_jobs), o.d_tab, o.d_tn_table, es, n, o.max_bands, o.lds_bytes, s, o.spec.rgb)); break;
    case Resample::Band: B_HIP(launch_resample_band(static_cast<const ResampleJob *>(o.d_jobs), o.d_tab, n, o.max_bands, o.lds_bytes, s, o.spec.rgb)); break;
    }
    if (o.route.runs) {  // (the images whose bands go in runs: their own launch, beside the band launch above)
        if (o.route.resample == Resample::Tensor)
            B_HIP(launch_resample_tensor_run(static_cast<const TensorJob *>(o.d_jobs) + n, o.d_tab, o.d_tn_table, o.d_bpr, es, n, o.max_runs, o.lds_bytes, s));
        else B_HIP(launch_resample_run(static_cast<const ResampleJob *>(o.d_jobs) + n, o.d_tab, o.d_bpr, n, o.max_runs, o.lds_bytes, s));
    }
    if (o.route.colour) {  // (the programs: behind the resample on the same stream, in place on what the warp launch reads)
        if (o.cl_sent) B_HIP(hipStreamWaitEvent(s, o.cl_sent, 0));  // (the jobs may have gone up on another stream than this one)
        B_HIP(launch_colour(o.d_cl_jobs, o.d_cl_scale, n, colour_strip_rows_knob(), s));
    }
    if (o.route.warp) {  // (the warp: behind the resample on the same stream, from the second intermediate arena into the output arena)
        const uint32_t tiles = (o.spec.w * o.spec.h + WP_NT - 1u) / WP_NT;
        const int32_t *tabs = reinterpret_cast<const int32_t *>(o.d_wp_jobs + (size_t)n * sizeof(WarpJob));
        if (o.wp_sent) B_HIP(hipStreamWaitEvent(s, o.wp_sent, 0));  // (the jobs may have gone up on another stream than this one)
        B_HIP(launch_warp(reinterpret_cast<const WarpJob *>(o.d_wp_jobs), tabs, o.d_tn_table, o.spec.tensor ? es : 0u, n, tiles, s));
    }
    return JPGPU_OK;
}

extern "C" {

int jpgpu_batch_set_flips(jpgpu_batch *b, const uint8_t *flips) {
    if (!b) return JPGPU_ERR_FORMAT;
    if (!b->o.spec.tensor) return set_err(b->err, JPGPU_ERR_UNSUPPORTED, "jpgpu_batch_set_flips: the batch has no tensor format");
    for (size_t i = 0; i < b->o.flips.size(); i++) b->o.flips[i] = flips && flips[i] ? 1 : 0;
    (b->o.route.warp ? b->o.wp_dirty : b->o.tn_dirty) = true;  // (a warped batch: the flip is a field of the WarpJobs)
    return JPGPU_OK;
}
int jpgpu_batch_set_warps(jpgpu_batch *b, const jpgpu_warp *warps) {
    if (!b) return JPGPU_ERR_FORMAT;
    OutputStage &o = b->o;
    if (!o.spec.warp) return set_err(b->err, JPGPU_ERR_UNSUPPORTED, "jpgpu_batch_set_warps: the batch has no warp (jpgpu_batch_create_warped)");
    for (size_t i = 0; warps && i < o.m.size(); i++)  // (one refused matrix refuses the call: nothing is changed)
        if (!warp_check(warps[i].m, o.spec.w, o.spec.h))
            return set_err(b->err, JPGPU_ERR_FORMAT, "jpgpu_batch_set_warps: image %zu: matrix (%g, %g, %g, %g, %g, %g) refused for %ux%u (jpgpu_warp_check)", i,
                           warps[i].m[0], warps[i].m[1], warps[i].m[2], warps[i].m[3], warps[i].m[4], warps[i].m[5], o.spec.w, o.spec.h);
    for (size_t i = 0; i < o.m.size(); i++) o.m[i] = warps ? warps[i] : kIdentity;
    o.wp_dirty = true;
    return JPGPU_OK;
}
int jpgpu_batch_set_colour_programs(jpgpu_batch *b, const jpgpu_colour_program *programs) {
    if (!b) return JPGPU_ERR_FORMAT;
    OutputStage &o = b->o;
    if (!o.route.colour) return set_err(b->err, JPGPU_ERR_UNSUPPORTED, "jpgpu_batch_set_colour_programs: the batch has no colour options (jpgpu_batch_create_coloured)");
    std::string why;
    for (size_t i = 0; programs && i < o.programs.size(); i++) {  // (one refused program refuses the call: nothing is changed)
        const int rc = colour_program_rule(o.spec, b->descs[i].ncomp, as_program(programs[i]), why);
        if (rc) return set_err(b->err, rc, "jpgpu_batch_set_colour_programs: image %zu: %s", i, why.c_str());
    }
    for (size_t i = 0; i < o.programs.size(); i++) o.programs[i] = programs ? as_program(programs[i]) : ColourProgram{};
    o.cl_dirty = true;
    return JPGPU_OK;
}
int jpgpu_colour_check(const jpgpu_colour_program *program) { return (program && colour_program_check(as_program(*program))) ? JPGPU_OK : JPGPU_ERR_FORMAT; }
int jpgpu_colour_point_lut(uint32_t op, float value, uint32_t mean, uint8_t *lut) {
    if (!lut || mean > 255u || op == CL_COLOR || op == CL_AUTOCONTRAST || op == CL_EQUALIZE || op >= CL_PIXEL_OPS || !colour_op_check(op, value)) return JPGPU_ERR_FORMAT;
    for (uint32_t v = 0; v < 256u; v++) lut[v] = (uint8_t)cl_point_value(op, value, mean, v);
    return JPGPU_OK;
}
int jpgpu_colour_autocontrast_lut(const uint32_t *h, uint8_t *lut) {
    if (!h || !lut) return JPGPU_ERR_FORMAT;
    double scale[256];
    colour_scale_table(scale);
    uint32_t lo, hi;
    cl_hist_range(h, lo, hi);
    for (uint32_t v = 0; v < 256u; v++) lut[v] = (uint8_t)cl_autocontrast_value(lo, hi, hi > lo ? scale[hi - lo] : 0.0, v);
    return JPGPU_OK;
}
int jpgpu_colour_equalize_lut(const uint32_t *h, uint8_t *lut) {
    if (!h || !lut) return JPGPU_ERR_FORMAT;
    for (uint32_t v = 0; v < 256u; v++) lut[v] = (uint8_t)cl_equalize_value(h, v);
    return JPGPU_OK;
}
// A program per image on the caller's pixels: the jobs and the scale table go up, the colour kernel runs on `stream`, and the call
// returns behind it.
int jpgpu_colour_apply(uint8_t *d_pixels, uint32_t n, uint32_t w, uint32_t h, const jpgpu_colour_program *programs, void *hip_stream) {
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if (n == 0) return JPGPU_OK;
    if (!d_pixels || !programs) return JPGPU_ERR_FORMAT;
    for (uint32_t i = 0; i < n; i++)  // (one refused program refuses the call: nothing is written)
        if (!colour_program_check(as_program(programs[i]))) return JPGPU_ERR_FORMAT;
    const size_t image = (size_t)3u * w * h;
    if (w == 0 || h == 0 || w > CL_MAX_SIDE || h > CL_MAX_SIDE || ((uintptr_t)d_pixels & 255u) != 0 || (image & 3u) != 0) return JPGPU_ERR_UNSUPPORTED;
    std::vector<ColourJob> jobs(n);
    for (uint32_t i = 0; i < n; i++) {
        const ColourProgram p = as_program(programs[i]);
        colour_job(jobs[i], d_pixels + (size_t)i * image, w, h, &p);
    }
    double scale[256];
    colour_scale_table(scale);
    const size_t jobs_bytes = (size_t)n * sizeof(ColourJob);
    uint8_t *d_block = nullptr;  // (the scale table, then the jobs)
    if (hipMalloc((void **)&d_block, sizeof scale + jobs_bytes) != hipSuccess) return JPGPU_ERR_IO;
    hipError_t e = hipMemcpyAsync(d_block, scale, sizeof scale, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_block + sizeof scale, jobs.data(), jobs_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = launch_colour(reinterpret_cast<const ColourJob *>(d_block + sizeof scale), reinterpret_cast<const double *>(d_block), n, colour_strip_rows_knob(), stream);
    const hipError_t done = hipStreamSynchronize(stream);  // (the host blocks above are read by now, whatever failed)
    (void)hipFree(d_block);
    return e == hipSuccess && done == hipSuccess ? JPGPU_OK : JPGPU_ERR_IO;
}
int jpgpu_oriented_window(uint32_t orientation, uint32_t w, uint32_t h, const jpgpu_window *oriented, uint32_t *oriented_w, uint32_t *oriented_h,
                          jpgpu_window *source) {
    if (!orient_valid(orientation) || w == 0 || h == 0 || w > 65535u || h > 65535u) return JPGPU_ERR_FORMAT;
    uint32_t ow, oh, sx, sy, sw, sh;
    oriented_size(orientation, w, h, ow, oh);
    if (oriented_w) *oriented_w = ow;
    if (oriented_h) *oriented_h = oh;
    const jpgpu_window wn = oriented ? *oriented : jpgpu_window{0, 0, 0, 0};
    if (!orient_source_window(orientation, w, h, wn.x, wn.y, wn.w, wn.h, sx, sy, sw, sh)) return JPGPU_ERR_FORMAT;
    if (source) *source = jpgpu_window{(uint16_t)sx, (uint16_t)sy, (uint16_t)sw, (uint16_t)sh};
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

}  // extern "C"
