/*
 * jpgpu.h — C ABI of the MI355X (gfx950) pixel-pipeline backend for image-rs/jpeg-decoder.
 *
 * This is the drop-in boundary: exactly what a `src/worker/hip.rs` backend of the crate
 * binds over FFI (see INTEGRATION.md for the Rust `extern "C"` block).  Plain pointers and
 * sizes only; no C++ / torch types.  Every entry point cites the reference interface
 * (paths relative to the reference crate root, v0.3.2) it replaces.
 *
 * Semantics are those of the crate's *scalar* path (`--features platform_independent`):
 * integer IDCT of src/idct.rs, upsamplers of src/upsampler.rs, colour conversion of
 * src/decoder.rs:1391-1508 — bit-exact, including i32 wrap-around on hostile input.
 *
 * Threading: a context object (worker / batch / decoder) is used by one thread at a time
 * (the crate holds its worker behind a RefCell, src/worker/mod.rs:44-46); different
 * contexts may be used concurrently from any threads.  Nothing unwinds across this ABI.
 */
#ifndef JPGPU_H
#define JPGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JPGPU_MAX_COMPONENTS 4 /* src/decoder.rs:21 MAX_COMPONENTS */

/* Status codes. 1..4 map one-to-one onto src/error.rs:16-48 Error::{Format, Unsupported,
 * Io, Internal}; the Rust shim turns them back into that enum. */
enum {
    JPGPU_OK = 0,
    JPGPU_ERR_FORMAT = 1,      /* Error::Format(String)            */
    JPGPU_ERR_UNSUPPORTED = 2, /* Error::Unsupported(..)           */
    JPGPU_ERR_IO = 3,          /* Error::Io (incl. device/runtime) */
    JPGPU_ERR_INTERNAL = 4,    /* Error::Internal / would-panic    */
    JPGPU_ERR_NO_DEVICE = 5,   /* no usable gfx950 device (maps to Error::Io) */
};

/* ColorTransform, src/decoder.rs:76-98 (same order). */
enum {
    JPGPU_CT_NONE = 0,
    JPGPU_CT_UNKNOWN = 1,
    JPGPU_CT_GRAYSCALE = 2,
    JPGPU_CT_RGB = 3,
    JPGPU_CT_YCBCR = 4,
    JPGPU_CT_CMYK = 5,
    JPGPU_CT_YCCK = 6,
    JPGPU_CT_JCS_BG_YCC = 7,
    JPGPU_CT_JCS_BG_RGB = 8,
};

/* parser::Component, src/parser.rs:76-89 (what RowData carries, src/worker/mod.rs:18-22). */
typedef struct jpgpu_component {
    uint8_t identifier;
    uint8_t horizontal_sampling_factor;
    uint8_t vertical_sampling_factor;
    uint8_t quantization_table_index;
    uint32_t dct_scale;                  /* 8 (full), 4, 2 or 1 */
    uint16_t size_width, size_height;    /* size       */
    uint16_t block_width, block_height;  /* block_size */
} jpgpu_component;

/* ---- library ------------------------------------------------------------------------ */
const char *jpgpu_version(void);
int jpgpu_device_count(int *count);            /* number of visible HIP devices */
const char *jpgpu_status_string(int status);
/* Opt-in, once, BEFORE the process's first HIP call (the HIP runtime reads its environment when it initialises): sets
 * GPU_MAX_HW_QUEUES=24 unless the variable is set already — jpgpu_pipeline_decode runs its sub-batches side by side on ~20 streams,
 * which the runtime otherwise folds onto 4 hardware queues.  Returns 1 if it set the variable, 0 if not.
 * Loading the library has no such side effect. */
int jpgpu_process_init(void);

/* ---- Worker: trait Worker, src/worker/mod.rs:24-35 ----------------------------------- */
/* One worker per decode() (WorkerScope, src/worker/mod.rs:44-95).  Planes live in HBM. */
typedef struct jpgpu_worker jpgpu_worker;

int jpgpu_worker_create(int device, jpgpu_worker **out); /* WorkerScopeInner::Hip(Default) */
void jpgpu_worker_destroy(jpgpu_worker *w);
const char *jpgpu_worker_last_error(const jpgpu_worker *w);
/* Name of the kernels the last jpgpu_compute_image of this worker ran: "generic" (planes -> pixels) or the fused kernel
 * of the frame's kind ("fused420", ... — coefficients -> pixels in one launch, taken when every component reached the
 * frame as a complete plane of coefficients at full scale through finish_plane). Diagnostics / tests. */
const char *jpgpu_worker_last_path(const jpgpu_worker *w);
/* Range class (0, 1 or 3: see jpgpu_batch_set_range_hint) the fused kernel of the last jpgpu_compute_image ran with; -1 if
 * that call took the generic kernels.  The class is worked out on the device from the frame's coefficients (one scan at HBM
 * speed in front of the kernel, nothing read back); this call reads it back (blocking).  Diagnostics / tests. */
int jpgpu_worker_last_class(jpgpu_worker *w);

/* Worker::start(RowData{index, component, quantization_table}) — src/worker/mod.rs:25,
 * src/worker/rayon.rs:40-49.  `quantization_table` is in natural (un-zigzagged) order. */
int jpgpu_worker_start(jpgpu_worker *w, uint32_t index, const jpgpu_component *component,
                       const uint16_t quantization_table[64]);

/* Worker::append_row((index, Vec<i16>)) — src/worker/mod.rs:26, src/worker/rayon.rs:71-132.
 * `len` must equal block_width * vertical_sampling_factor * 64 (the reference asserts).
 * The data is consumed (copied to pinned staging) before the call returns. */
int jpgpu_worker_append_row(jpgpu_worker *w, uint32_t index, const int16_t *coefficients,
                            size_t len);

/* Worker::append_rows(iterator) — src/worker/mod.rs:29-34, src/worker/rayon.rs:140-185:
 * `n_rows` consecutive MCU rows stored back to back. */
int jpgpu_worker_append_rows(jpgpu_worker *w, uint32_t index, const int16_t *coefficients,
                             size_t n_rows);

/* Worker::get_result(index) -> Vec<u8> — src/worker/mod.rs:27, src/worker/rayon.rs:134-137.
 * Runs the IDCT of everything appended, copies the plane (block_w*block_h*dct_scale^2
 * bytes) to `dst`, and (mem::take) forgets the host-visible result; the device plane is
 * kept for jpgpu_compute_image under the same index until the next start(). */
int jpgpu_worker_get_result(jpgpu_worker *w, uint32_t index, uint8_t *dst, size_t cap,
                            size_t *len);

/* Device-resident variant: finish the plane but do not download it.  `plane_slot` is the
 * frame-level component position it will have in jpgpu_compute_image (decode_scan uses
 * scan-local indices, src/decoder.rs:848-852,1072-1075). */
int jpgpu_worker_finish_plane(jpgpu_worker *w, uint32_t index, uint32_t plane_slot);

/* compute_image, src/decoder.rs:1300-1336 == 1-component compaction + compute_image_parallel
 * (src/worker/mod.rs:97-128, src/worker/rayon.rs:193-219).  If host_planes is NULL the
 * device planes left by get_result / finish_plane are used (slot i = components[i]);
 * otherwise host_planes[i] (plane bytes as returned by get_result) are uploaded first.
 * Output: out_w*out_h*ncomp bytes (1 component: size_w*size_h). */
int jpgpu_compute_image(jpgpu_worker *w, const jpgpu_component *components, uint32_t ncomp,
                        const uint8_t *const *host_planes, uint16_t out_w, uint16_t out_h,
                        int color_transform, uint8_t *dst, size_t cap, size_t *len);

/* ---- Batch: N independent images per launch (no reference counterpart: the crate decodes
 * one image per Decoder; this is how a batch shards one-image-per-task across a GPU) ------ */
typedef struct jpgpu_image_desc {
    uint32_t ncomp;
    jpgpu_component components[JPGPU_MAX_COMPONENTS];
    uint16_t quantization_tables[JPGPU_MAX_COMPONENTS][64]; /* per component, natural order */
    uint16_t out_w, out_h;   /* FrameInfo::output_size */
    int32_t color_transform; /* determine_color_transform() result */
} jpgpu_image_desc;

typedef struct jpgpu_batch jpgpu_batch;

enum {
    JPGPU_BATCH_DEFAULT = 0,
    JPGPU_BATCH_EXTERNAL_BUFFERS = 1, /* caller binds device memory (e.g. torch tensors)   */
    JPGPU_BATCH_FORCE_GENERIC = 2,    /* never take the fused fast paths (two-kernel path)  */
    JPGPU_BATCH_ASSUME_HOSTILE = 4,   /* skip the range scan: always use the exact 32-bit path */
    JPGPU_BATCH_RGB_OUTPUT = 8,       /* with an output size: every image gives three channels (see below) */
    /* bits 8..11: the resample filter of a batch with an output size, JPGPU_BATCH_FILTER(JPGPU_FILTER_*) (see "Resample filters") */
};

int jpgpu_batch_create(int device, const jpgpu_image_desc *descs, uint32_t n_images,
                       uint32_t flags, jpgpu_batch **out);
/* A window of each image's output: (x, y, w, h) in the pixel grid of the image's output (out_w x out_h, after Decoder::scale;
 * for one component the component's size, as compute_image has it).  w == 0 or h == 0: the whole image. */
typedef struct jpgpu_window {
    uint16_t x, y, w, h;
} jpgpu_window;
/* jpgpu_batch_create with a window per image (`windows` NULL: exactly jpgpu_batch_create).  The pixels of image i are then the
 * window's rows and columns of the whole decode, in the same pixel format, packed (row pitch w * ncomp bytes):
 *   interleaving colour functions        full.reshape(H, W, nc)[y:y+h, x:x+w]
 *   ColorTransform None, > 1 component   full.reshape(H, nc, W)[y:y+h, :, x:x+w]   (color_no_convert: planar within a row)
 * jpgpu_batch_out_bytes / out_offset, the output arena and jpgpu_batch_download hold the window's bytes; the coefficient arena
 * stays whole-image.  A window that covers the whole image is no window (same route, same kernels, same bytes).  Windowed images
 * run a kernel of their own (jpgpu_batch_path: "window", or "mixed" with other images) with exact arithmetic at every scale.
 * A window that does not lie inside its image fails creation with JPGPU_ERR_FORMAT; a hand-made descriptor the window planner
 * refuses (components at different dct_scales) with JPGPU_ERR_UNSUPPORTED and the reason in jpgpu_batch_last_error. */
int jpgpu_batch_create_windowed(int device, const jpgpu_image_desc *descs, const jpgpu_window *windows, uint32_t n_images,
                                uint32_t flags, jpgpu_batch **out);
/* ---- A fixed output size: every image resampled to out_w x out_h on the device -----------------------------------------------
 * jpgpu_batch_create_windowed (`windows` may be NULL) with an output size, out_w and out_h in 1..2048.  The pixels of image i are
 * the resample to out_w x out_h of what image i gives without it: its window, or its whole output when it has none (the grid after
 * Decoder::scale; the colour transform is unchanged).  Every image's result is out_h * out_w * ncomp bytes, interleaved and packed.
 * jpgpu_batch_out_bytes / out_offset, the output arena (the caller's with EXTERNAL_BUFFERS), jpgpu_batch_out_arena_bytes and
 * jpgpu_batch_download hold the RESIZED pixels; the pixels the batch's other kernels write go, by the same routes and launches, to an
 * intermediate arena the batch always owns, and one more launch behind them on the same stream resamples every image
 * (jpgpu_batch_path gains the suffix "+resize").  An out_w or out_h of 0 or above 2048 fails creation with JPGPU_ERR_FORMAT; planar
 * output (ColorTransform None with more than one component) with JPGPU_ERR_UNSUPPORTED.
 *
 * The arithmetic is the 8-bit integer bilinear resample with antialiasing that Pillow's Image.resize(size, BILINEAR) performs on the
 * cropped image — crop, then resize: nothing outside the window is read.  PRECISION_BITS = 22.  Per axis, from in_size to out_size,
 * in IEEE double:
 *   1. scale = in_size / out_size, fs = max(scale, 1.0), support = fs, ksize = ceil(support) * 2 + 1, ss = 1.0 / fs.
 *   2. for output index xx: center = (xx + 0.5) * scale, xmin = max((int)(center - support + 0.5), 0),
 *      xmax = min((int)(center + support + 0.5), in_size), n = xmax - xmin.
 *   3. for x < n: a = |(x + xmin - center + 0.5) * ss|, w[x] = a < 1 ? 1 - a : 0; ww = the sum of w[x] in index order.
 *   4. k[x] = (int)(w[x] / ww * 2^22 + 0.5)   (never negative).
 *   5. one pass: out = clamp((2^21 + sum p[xmin + x] * k[x]) >> 22, 0, 255) in 32-bit integers (the sum stays below 2^31).
 *   6. the horizontal pass runs first and is rounded to u8; the vertical pass runs on its result.
 * An axis whose size does not change yields the identity (k = {2^22, 0}).  One known difference from Pillow: its Python wrapper runs
 * the vertical pass first when H > 100 W and out_h < H (+-1 on such images); this library never does. */
int jpgpu_batch_create_resized(int device, const jpgpu_image_desc *descs, const jpgpu_window *windows, uint16_t out_w, uint16_t out_h,
                               uint32_t n_images, uint32_t flags, jpgpu_batch **out);
/* The tables of one axis as the batch computes them (pure host function, no device needed): `bounds` receives out_size pairs
 * (xmin, n), `coefs` out_size x ksize int32 weights, zero beyond n; *ksize the row length.  With `bounds` and `coefs` NULL only
 * *ksize is set (to size the buffers).  in_size and out_size are 1..65535; anything else is JPGPU_ERR_FORMAT. */
int jpgpu_resample_coefficients(uint32_t in_size, uint32_t out_size, int32_t *bounds, int32_t *coefs, uint32_t *ksize);
/* ---- Resample filters: Pillow's BOX, BILINEAR, HAMMING, BICUBIC and LANCZOS ---------------------------------------------------------
 * JPGPU_BATCH_FILTER(f) in the `flags` of jpgpu_batch_create_resized / _create_tensor / _create_placed picks the filter of every
 * resample of the batch (every image, both axes; a placed image's resample to rw x rh).  0 = JPGPU_FILTER_BILINEAR, so flags without
 * the bits give what they always gave — tables, kernels, bytes and jpgpu_batch_path.  With another filter the result is Pillow's
 * Image.resize(size, F) on the cropped image: rules 1-6 above with three changes.
 *   1'. support = S_F * fs with S_F = 1 (BILINEAR), 0.5 (BOX), 1 (HAMMING), 2 (BICUBIC), 3 (LANCZOS); ksize = ceil(support) * 2 + 1; xmin,
 *       xmax, n and ss as in rules 1-2 with this support.
 *   3'. w[x] = f((x + xmin - center + 0.5) * ss) on the SIGNED argument, in IEEE double, one operation per statement (no FMA), sin and
 *       cos the C library's:
 *         BOX       1 if -0.5 < x <= 0.5, else 0
 *         BILINEAR  x = |x|;  x < 1 ? 1 - x : 0
 *         HAMMING   x = |x|;  x == 0: 1;  x >= 1: 0;  x = x * pi;  sin(x) / x * (0.54f + 0.46f * cos(x)) — the two constants are FLOAT
 *                   literals promoted to double
 *         BICUBIC   a = -0.5;  x = |x|;  x < 1: ((a + 2) x - (a + 3)) x x + 1;  x < 2: (((x - 5) x + 8) x - 4) a;  else 0
 *         LANCZOS   -3 <= x < 3: sinc(x) * sinc(x / 3), else 0;  sinc(0) = 1, sinc(x) = sin(x pi) / (x pi)
 *   4'. v = w[x] / ww (w[x] itself where ww == 0);  k[x] = v < 0 ? (int)(-0.5 + v * 2^22) : (int)(0.5 + v * 2^22).  Weights can be
 *       negative; both passes clamp to 0..255 as rule 5 states; 255 * sum |k[x]| + 2^21 stays below 2^31 (tests/test_filters.py sweeps it),
 *       so partial sums are exact in 32 bits in any order.
 * An axis whose size does not change yields k = {2^22} under every filter.  jpgpu_batch_path names a filter other than BILINEAR behind
 * "+resize": "+resize:bicubic", "+resize:lanczos+tensor"; and "+roll" at its end where some image's resample runs in runs of bands (BICUBIC
 * and LANCZOS plans whose row bands overlap by more than 1.3: workgroups that keep the shared source rows in LDS — same bytes).  Refusals: a filter other than 0 on jpgpu_batch_create / _create_windowed (no
 * output size): JPGPU_ERR_UNSUPPORTED, as RGB output; an id above 4: JPGPU_ERR_FORMAT. */
enum { JPGPU_FILTER_BILINEAR = 0, JPGPU_FILTER_BOX = 1, JPGPU_FILTER_HAMMING = 2, JPGPU_FILTER_BICUBIC = 3, JPGPU_FILTER_LANCZOS = 4 };
#define JPGPU_BATCH_FILTER(f) (((uint32_t)(f) & 15u) << 8)
/* jpgpu_resample_coefficients / jpgpu_resample_coefficients_range (below) under a filter; filter 0 gives exactly what they give.  An
 * id above 4: JPGPU_ERR_FORMAT. */
int jpgpu_resample_coefficients_filtered(uint32_t filter, uint32_t in_size, uint32_t out_size, int32_t *bounds, int32_t *coefs, uint32_t *ksize);
int jpgpu_resample_coefficients_range_filtered(uint32_t filter, uint32_t in_size, uint32_t out_size, uint32_t first, uint32_t count, int32_t *bounds,
                                               int32_t *coefs, uint32_t *ksize);
/* ---- A tensor output: every image resampled, normalised and written channel-first, as the model reads it -----------------------
 * jpgpu_batch_create_resized with a tensor format.  The output of image i is ncomp x out_h x out_w elements of `dtype`, planar (CHW)
 * and packed:
 *     elem(c, r, x) = T[c][ u8(r, flip_i ? out_w - 1 - x : x, c) ]
 * u8 is the resized output of that image exactly as jpgpu_batch_create_resized defines it; flip_i is a flag per image
 * (jpgpu_batch_set_flips; applied last, to the resampled image: a pure mirror of columns); T is a table of ncomp x 256 elements made
 * on the host in IEEE single precision, one operation per statement:
 *     a = (float)v / 255.0f;   b = a - mean[c];   t = b / std[c];
 *     T[c][v] = t (f32), t rounded to nearest even to binary16 (f16), t rounded to nearest even to bfloat16 (bf16)
 * — what torch's arange(256, uint8).to(float32).div(255).sub_(mean).div_(std) (then .to(dtype)) gives on the CPU, bit for bit.  The
 * device looks the table up and does no float arithmetic: the result is exact by construction.  There is no resized u8 image in this
 * mode: the resample's vertical pass writes the tensor (jpgpu_batch_path ends in "+resize+tensor").
 *
 * jpgpu_batch_out_bytes(i) is ncomp * out_h * out_w * sizeof(dtype); jpgpu_batch_out_offset / the output arena (the caller's with
 * EXTERNAL_BUFFERS) / jpgpu_batch_download hold the tensor.  Image offsets are 256-byte aligned as everywhere: images whose tensor
 * is a multiple of 256 bytes — 3 x 224 x 224 in any of the three dtypes — follow each other without a gap, so the arena of N such
 * images IS one contiguous N x 3 x 224 x 224 tensor.
 *
 * Refusals: a std[c] that is 0 or not finite, or a mean[c] that is not finite, for c < ncomp of any image of the call, an unknown
 * dtype, reserved != 0, a NULL format or an output size of 0: JPGPU_ERR_FORMAT; planar ColorTransform None images:
 * JPGPU_ERR_UNSUPPORTED, as with an output size. */
enum { JPGPU_TENSOR_F32 = 1, JPGPU_TENSOR_F16 = 2, JPGPU_TENSOR_BF16 = 3 };
typedef struct jpgpu_tensor_format {
    uint32_t dtype;    /* JPGPU_TENSOR_* */
    uint32_t reserved; /* must be 0 */
    float mean[4];
    float std[4];
} jpgpu_tensor_format;
int jpgpu_batch_create_tensor(int device, const jpgpu_image_desc *descs, const jpgpu_window *windows, uint16_t out_w, uint16_t out_h,
                              const jpgpu_tensor_format *format, uint32_t n_images, uint32_t flags, jpgpu_batch **out);
/* ---- RGB output: three channels for every image of a resized / tensor batch (JPGPU_BATCH_RGB_OUTPUT) -----------------------------
 * With the flag, jpgpu_batch_create_resized and jpgpu_batch_create_tensor give every image three channels — out_h * out_w * 3 bytes,
 * interleaved, or 3 x out_h x out_w elements — so the arena of N images to 224 x 224 IS one N x 3 x 224 x 224 tensor whatever the
 * files hold.  The result is convert, then crop, then resample — Image.open(f).convert("RGB") followed by the crop and resize:
 *     rgb(src) -> the resample above, unchanged -> (the table lookup and flip above, unchanged, with 3 channels)
 * where src is what the image gives without an output size (its window, or all of it, nc_src channels) and
 *   nc_src == 3 (YCbCr, RGB):  rgb(src) = src.
 *   nc_src == 1 (gray):        R = G = B = v.
 *   nc_src == 4 (CMYK, YCCK; ink amounts, 0 = no ink — Pillow's mode "CMYK"): Pillow's cmyk2rgb per pixel, in 32-bit integers:
 *       nk = 255 - K;   for X in (C, M, Y):  t = X * nk + 128;  md = ((t >> 8) + t) >> 8;  out = nk - md
 *     (= (2 (255 - X)(255 - K) + 255) / 510 rounded down; no clamp: md <= nk).  Not linear: applied to the source pixels BEFORE the
 *     horizontal pass.
 * Only the resample launch differs (jpgpu_batch_path gains "+rgb" before "+resize"): the batch's other kernels write L8 / RGB24 /
 * CMYK32 to the intermediate arena as without the flag.  A tensor format's mean[c] and std[c] are checked for c < 3 and the table is
 * jpgpu_tensor_table(format, 3, ...) for every image: a gray image's three planes differ through T[c].  Without the flag nothing
 * changes.  Refusals: the flag on jpgpu_batch_create / _create_windowed (no output size): JPGPU_ERR_UNSUPPORTED with the reason in
 * jpgpu_batch_last_error; planar ColorTransform None images stay JPGPU_ERR_UNSUPPORTED. */
/* The flip flag of every image (`flips`: n_images bytes, non-zero = mirrored; NULL: none) from the next jpgpu_batch_decode on: a
 * field of the image's job record, sent with the job tables.  Never changes a size or an offset.  JPGPU_ERR_UNSUPPORTED on a batch
 * without a tensor format. */
int jpgpu_batch_set_flips(jpgpu_batch *b, const uint8_t *flips);
/* The table T of a format for images of `nc` channels (1..4) as the batch computes it (pure host function, no device needed): `table`
 * receives nc x 256 elements of the format's dtype (bf16 / f16 as their 16-bit patterns).  A refused format: JPGPU_ERR_FORMAT. */
int jpgpu_tensor_table(const jpgpu_tensor_format *format, uint32_t nc, void *table);
/* ---- Resize, then crop or pad: a placement per image in the fixed output size ------------------------------------------------------
 * jpgpu_batch_create_resized / _create_tensor (`format` NULL: u8) with a placement per image: the image's source is resampled to a
 * size of its own, rw x rh, and laid with its top-left pixel at (x, y) into the out_w x out_h output.  What falls outside is cropped,
 * what the image does not cover is `fill`.  With R the resample of the image's source to rw x rh, the output of image i is
 *     out(Y, X, c) = R(Y - y, X - x, c)   if 0 <= X - x < rw and 0 <= Y - y < rh
 *                  = fill[c]              otherwise
 *   - the source is the image's window, or its whole output, in the grid after the DCT scale — the source of the fixed output size,
 *     after the RGB conversion when JPGPU_BATCH_RGB_OUTPUT is set;
 *   - R follows rules 1-6 of jpgpu_batch_create_resized (under the batch's filter, JPGPU_BATCH_FILTER) with out_size = rw / rh, the
 *     horizontal pass first;
 *   - `fill` is four bytes per batch in the output's channel order (NULL: zeros);
 *   - the Pillow equivalent is canvas = Image.new(mode, (out_w, out_h), fill); canvas.paste(src.resize((rw, rh), BILINEAR), (x, y));
 *   - with a tensor format the element is T[c][out(r, flip ? out_w - 1 - x : x, c)]: a filled element is T[c][fill[c]] — what Pad(fill)
 *     in front of Normalize gives — and the flip mirrors the finished canvas, padding included;
 *   - the known difference from Pillow stays as documented: sources with H > 100 W and rh < H.
 * rw == 0 or rh == 0 means "none" = (out_w, out_h, 0, 0).  Every output pixel of the two-pass resample depends on its own row and column
 * of the tables only: the visible part is computed from the sub-range of the tables the output covers
 * (jpgpu_resample_coefficients_range), nothing outside it.  Output sizes, offsets, the arena, jpgpu_batch_download,
 * JPGPU_BATCH_EXTERNAL_BUFFERS, jpgpu_batch_set_flips and caller streams are those of the fixed output size.  jpgpu_batch_path gains
 * "+place" before "+resize" exactly when some image has a placement other than (out_w, out_h, 0, 0); `placements` NULL, or no such
 * image, IS jpgpu_batch_create_resized / _create_tensor: the same kernels and path.
 * Refusals: a placement must show at least one pixel — x < out_w, x + rw > 0, y < out_h, y + rh > 0 — else JPGPU_ERR_FORMAT; planar
 * ColorTransform None images stay JPGPU_ERR_UNSUPPORTED. */
typedef struct jpgpu_placement {
    uint16_t rw, rh; /* the size the image's source is resampled to, 1..65535 each; rw == 0 or rh == 0: "none" = (out_w, out_h, 0, 0) */
    int32_t x, y;    /* where that resampled image's top-left pixel lies in the out_w x out_h output; negative: cropped */
} jpgpu_placement;
int jpgpu_batch_create_placed(int device, const jpgpu_image_desc *descs, const jpgpu_window *windows, const jpgpu_placement *placements,
                              const uint8_t *fill, uint16_t out_w, uint16_t out_h, const jpgpu_tensor_format *format, uint32_t n_images,
                              uint32_t flags, jpgpu_batch **out);
/* Entries [first, first + count) of the tables jpgpu_resample_coefficients(in_size, out_size, ...) gives (pure host function): bounds
 * receives 2 * count, coefs count * ksize words, ksize = jpgpu_resample_coefficients' for (in_size, out_size).  Computed per entry
 * from the same statements: an axis of 65535 entries is never tabulated whole.  first + count > out_size: JPGPU_ERR_FORMAT. */
int jpgpu_resample_coefficients_range(uint32_t in_size, uint32_t out_size, uint32_t first, uint32_t count, int32_t *bounds, int32_t *coefs,
                                      uint32_t *ksize);
/* The placement of a source of src_w x src_h in an output of out_w x out_h under a rule (pure host function):
 *   JPGPU_FIT_STRETCH: (out_w, out_h, 0, 0).
 *   JPGPU_FIT_SHORTER_SIDE_CROP — torchvision's Resize(size) then CenterCrop((out_h, out_w)): w <= h: rw = size, rh = size * h / w;
 *     else rh = size, rw = size * w / h (64-bit integer division).  Per axis, d = r - out: d >= 0: the offset is -round_half_even(d / 2);
 *     d < 0: the offset is (out - r) / 2 rounded down.  A side above 65535: JPGPU_ERR_FORMAT.
 *   JPGPU_FIT_LETTERBOX, in IEEE double, one operation per statement: r = min(out_w / w, out_h / h); rw = max(1, rint(w r)),
 *     rh = max(1, rint(h r)), each capped at the output's; x = (int)rint((out_w - rw) / 2.0 - 0.1), y likewise (rint: to nearest even).
 * `fill` is what the caller passes on to jpgpu_batch_create_placed.  An unknown mode, reserved != 0, a zero size (mode 1: `size` too):
 * JPGPU_ERR_FORMAT. */
enum { JPGPU_FIT_STRETCH = 0, JPGPU_FIT_SHORTER_SIDE_CROP = 1, JPGPU_FIT_LETTERBOX = 2 };
typedef struct jpgpu_fit {
    uint32_t mode; /* JPGPU_FIT_* */
    uint32_t size; /* JPGPU_FIT_SHORTER_SIDE_CROP: what the shorter side is resampled to */
    uint8_t fill[4];
    uint32_t reserved; /* 0 */
} jpgpu_fit;
int jpgpu_fit_placement(const jpgpu_fit *fit, uint32_t src_w, uint32_t src_h, uint32_t out_w, uint32_t out_h, jpgpu_placement *out);
/* ---- Affine warps behind the fixed output size: rotate, shear, translate per image --------------------------------
 * jpgpu_batch_create_placed with a warp stage behind the resample.  With R the image's u8 result of out_w x out_h, exactly as the same
 * batch without a warp defines it (placement fill included), and F the image's flip (tensor batches only):
 *     out(Y, X, c)  = Warp_i( F ? mirror_columns(R) : R )(Y, X, c)        u8 batches: these bytes, interleaved
 *     elem(c, Y, X) = T[c][ out(Y, X, c) ]                                 tensor batches, CHW
 * The flip comes BEFORE the warp (torchvision's order: flip, then the policy).  Warp is Pillow's
 * Image.transform((out_w, out_h), Image.AFFINE, m, resample, fillcolor=fill) of the source S = R (W x H = out_w x out_h): m[0..5] is the
 * inverse map, output pixel -> source position; the output starts as `fill` — the warp's own, separate from a placement's — and a tensor
 * element outside the source is T[c][fill[c]].
 *   N  — JPGPU_WARP_NEAREST, m[1] != 0 || m[3] != 0: 16.16 fixed point.  FIX(v) = (int)floor(v * 65536.0 + 0.5); a0, a1, a3, a4 = FIX of
 *        m[0], m[1], m[3], m[4]; a2 = FIX(m[2] + m[0]*0.5 + m[1]*0.5), a5 = FIX(m[5] + m[3]*0.5 + m[4]*0.5) (doubles, one operation per
 *        statement, left to right); xi = (a2 + X a0 + Y a1) >> 16, yi = (a5 + X a3 + Y a4) >> 16 (arithmetic shifts);
 *        0 <= xi < W && 0 <= yi < H: out = S[yi][xi], else the fill stays.
 *   N-sep — JPGPU_WARP_NEAREST, m[1] == 0 && m[3] == 0: an index per axis, a sequential sum of doubles (jpgpu_warp_nearest_axis):
 *        xo = m[2] + m[0]*0.5; for X = 0 .. out_w - 1: xs[X] = xo < 0.0 ? -1 : (int)xo, then xo += m[0]; ys likewise from m[5], m[4];
 *        out = S[ys[Y]][xs[X]] where both indices are in range.  (Other pixels than rule N gives, as in Pillow.)
 *   B  — JPGPU_WARP_BILINEAR, any matrix: IEEE double, no fused multiply-add.  xin = X + 0.5, yin = Y + 0.5;
 *        xo = (m0 xin + m1 yin) + m2, yo likewise; xo < 0 || xo >= W || yo < 0 || yo >= H: the fill stays; else xo -= 0.5, yo -= 0.5,
 *        x = floor(xo), y = floor(yo), dx = xo - x, dy = yo - y; x0 = clamp(x, 0, W-1), x1 = clamp(x+1, 0, W-1), r0 = clamp(y, 0, H-1);
 *        per channel v1 = p[r0][x0] + (p[r0][x1] - p[r0][x0]) dx; v2 the same on row y+1 if 0 <= y+1 < H, else v1;
 *        v = v1 + (v2 - v1) dy; out = (uint8)v, truncated.
 * A matrix is refused (jpgpu_warp_check: JPGPU_ERR_FORMAT) when a coefficient is not finite, |m[0]|, |m[1]|, |m[3]| or |m[4]| is above
 * 16000, or at a corner (X, Y) of (0,0), (out_w,0), (0,out_h), (out_w,out_h) |X m0 + Y m1 + m2| or |X m3 + Y m4 + m5| is above 32000:
 * inside these bounds every sum of rule N fits 32 bits.
 * `warp` NULL IS jpgpu_batch_create_placed: same kernels, bytes and path.  Otherwise every image starts with the identity; the batch's
 * resample launch is the u8 one of the same arguments and writes an arena the batch owns, one more launch behind it warps into the
 * output arena.  jpgpu_batch_path is the u8 batch's path, then "+warp" or "+warp:bilinear", then "+tensor" with a format.  A warp needs
 * an output size (JPGPU_ERR_FORMAT); planar ColorTransform None images stay JPGPU_ERR_UNSUPPORTED; an unknown filter or reserved != 0
 * is JPGPU_ERR_FORMAT. */
enum { JPGPU_WARP_NEAREST = 0, JPGPU_WARP_BILINEAR = 1 };
typedef struct jpgpu_warp {
    double m[6];
} jpgpu_warp;
typedef struct jpgpu_warp_options {
    uint32_t filter; /* JPGPU_WARP_NEAREST 0, JPGPU_WARP_BILINEAR 1 */
    uint8_t fill[4];
    uint32_t reserved; /* 0 */
} jpgpu_warp_options;
int jpgpu_batch_create_warped(int device, const jpgpu_image_desc *descs, const jpgpu_window *windows, const jpgpu_placement *placements,
                              const uint8_t *fill, uint16_t out_w, uint16_t out_h, const jpgpu_tensor_format *format, const jpgpu_warp_options *warp,
                              uint32_t n_images, uint32_t flags, jpgpu_batch **out);
/* The matrix of every image (`warps`: n_images entries; NULL: identities) from the next jpgpu_batch_decode enqueued on: fields of the
 * images' job records, sent with them on the decode's stream (a decode already enqueued keeps its matrices: "Batch calls on caller
 * streams" below).  One refused matrix refuses the call (JPGPU_ERR_FORMAT) and nothing is changed.  JPGPU_ERR_UNSUPPORTED on a batch
 * without a warp. */
int jpgpu_batch_set_warps(jpgpu_batch *b, const jpgpu_warp *warps);
/* Pure host functions (no device needed): the refusal rule above for an output of out_w x out_h (JPGPU_OK / JPGPU_ERR_FORMAT), and the
 * N-sep index table of one axis — idx[X] for X < out_size from the scale a (m[0] / m[4]) and the offset b (m[2] / m[5]); a position no
 * int holds gives INT32_MAX, one that is no number -1. */
int jpgpu_warp_check(const jpgpu_warp *warp, uint32_t out_w, uint32_t out_h);
int jpgpu_warp_nearest_axis(double a, double b, uint32_t out_size, int32_t *idx);
/* ---- EXIF orientation in front of the fixed output size ------------------------------------------------------------
 * jpgpu_batch_create_warped with an orientation per image (`orientations`: n_images bytes, each 1..8).  Let S be what image i gives the
 * resample without it: its whole output in the grid after the DCT scale, H x W x nc interleaved.  The oriented image O is Pillow's
 * Image.transpose(method) under ImageOps.exif_transpose's mapping:
 *     o  Pillow            O's size   O[y][x]
 *     1  none              W x H      S[y][x]
 *     2  FLIP_LEFT_RIGHT   W x H      S[y][W-1-x]
 *     3  ROTATE_180        W x H      S[H-1-y][W-1-x]
 *     4  FLIP_TOP_BOTTOM   W x H      S[H-1-y][x]
 *     5  TRANSPOSE         H x W      S[x][y]
 *     6  ROTATE_270        H x W      S[H-1-x][y]
 *     7  TRANSVERSE        H x W      S[H-1-x][W-1-y]
 *     8  ROTATE_90         H x W      S[x][W-1-y]
 * With an orientation, everything the output stage defines on "the image" is defined on O: the window is (x, y, w, h) inside O, checked
 * against O's size; the fit rules and jpgpu_fit_placement take the oriented window's size; the RGB conversion, the resample (the
 * horizontal pass first, on O's rows), placement, flip, warp and tensor table follow unchanged.  In Pillow's terms:
 * ImageOps.exif_transpose(Image.open(f)), then .convert("RGB"), then the crop, the resize and so on, as documented above.
 * On the host the oriented window is mapped back to the window of S whose orientation it is (jpgpu_oriented_window); the batch's pixel
 * routes decode that source window as ever — the window rule applies to it — and one launch behind them, in front of the resample
 * launch on the same stream, rewrites the source window of every image with o != 1, oriented and packed, into a second arena the batch
 * owns, where that image's resample reads.  Images with o == 1 are not touched.  jpgpu_batch_path gains "+orient" in front of "+rgb" /
 * "+place" / "+resize".  `orientations` NULL, or all ones, IS jpgpu_batch_create_warped: the same kernels, launches, bytes and path.
 * Refusals: a value outside 1..8: JPGPU_ERR_FORMAT; orientations other than 1 without an output size: JPGPU_ERR_UNSUPPORTED with the
 * reason in jpgpu_batch_last_error, as RGB output; planar ColorTransform None images stay JPGPU_ERR_UNSUPPORTED.
 * Differences from Pillow: the orientation is what the caller passes — jpgpu_exif_orientation reads the EXIF tag alone, where
 * ImageOps.exif_transpose falls back to the XMP packet's tiff:Orientation when the file has no EXIF tag: XMP is ignored here. */
int jpgpu_batch_create_oriented(int device, const jpgpu_image_desc *descs, const jpgpu_window *windows, const jpgpu_placement *placements,
                                const uint8_t *fill, uint16_t out_w, uint16_t out_h, const jpgpu_tensor_format *format,
                                const jpgpu_warp_options *warp, const uint8_t *orientations, uint32_t n_images, uint32_t flags, jpgpu_batch **out);
/* Pure host functions (no device needed).  jpgpu_oriented_window: for a source of w x h (1..65535 each) under `orientation`, O's size
 * into *oriented_w / *oriented_h and the window `oriented` of O (NULL, or w == 0 or h == 0: all of it, which stays "all") as the window
 * of S into *source; any output may be NULL.  An orientation outside 1..8, a size of 0 or a window outside O: JPGPU_ERR_FORMAT.
 * jpgpu_exif_orientation: the orientation an EXIF blob states — `exif` is the payload behind "Exif\0\0" (jpgpu_decoder_exif_data): the
 * TIFF header ("II" or "MM", magic 42), IFD0's offset, its 12-byte entries, tag 0x0112 of type SHORT and count 1 with a value of 1..8.
 * Anything else — no EXIF (NULL or len 0), a truncated or out-of-bounds IFD, another type or count, a value outside 1..8 — gives 1,
 * never an error; every read is checked against len. */
int jpgpu_oriented_window(uint32_t orientation, uint32_t w, uint32_t h, const jpgpu_window *oriented, uint32_t *oriented_w, uint32_t *oriented_h,
                          jpgpu_window *source);
uint32_t jpgpu_exif_orientation(const uint8_t *exif, size_t len);
/* ---- Colour operations behind the fixed output size: a program of Pillow operations per image ---------------------
 * jpgpu_batch_create_oriented with a colour stage behind the resample.  With R the image's u8 result of out_w x out_h, exactly as the
 * same batch without colour defines it (RGB conversion, orientation, resample and placement fill included), and a program of n <= 4
 * operations per image:
 *     C             = op_{n-1}( ... op_1( op_0( R ) ) )                     n == 0: C = R
 *     out(Y, X, c)  = Warp_i( F ? mirror_columns(C) : C )(Y, X, c)          warp and flip as above; absent: the identity
 *     elem(c, Y, X) = T[c][ out(Y, X, c) ]                                  tensor batches
 * Colour comes BEFORE the warp (a warp's fill is not recoloured); a placement's fill is part of R, is seen by the statistics and is
 * recoloured, as Pillow does on the pasted canvas.  Each operation works on the current image P (u8, H x W x 3); statistics are those of
 * the current P:
 *     0 IDENTITY      -            P
 *     1 BRIGHTNESS    factor f     blend(0, p, f) per channel value                      ImageEnhance.Brightness(P).enhance(f)
 *     2 CONTRAST      f            blend(m, p, f), m the image's mean                    ImageEnhance.Contrast(P).enhance(f)
 *     3 COLOR         f            blend(L(px), p, f) per pixel (f = 0: grayscale)       ImageEnhance.Color(P).enhance(f)
 *     4 SOLARIZE      threshold t  p < t ? p : 255 - p          t an integer 0..256      ImageOps.solarize(P, t)
 *     5 POSTERIZE     bits b       p & ~(2^(8-b) - 1)           b an integer 1..8        ImageOps.posterize(P, b)
 *     6 INVERT        -            255 - p                                               ImageOps.invert(P)
 *     7 AUTOCONTRAST  -            per channel                                           ImageOps.autocontrast(P)   (cutoff 0)
 *     8 EQUALIZE      -            per channel                                           ImageOps.equalize(P)
 *   blend(a, b, f): IEEE float32, the product and the sum rounded once each, no fused multiply-add: t = (float)a + f * (float)(b - a);
 *     0 <= f <= 1: (uint8)(int)t (truncated); otherwise t <= 0: 0, t >= 255: 255, else (uint8)(int)t.
 *   L(px) = (R 19595 + G 38470 + B 7471 + 0x8000) >> 16.   m = (2 s + n) / (2 n) in integers, s the sum of L over the n = W H pixels.
 *   AUTOCONTRAST, per channel: lo / hi the least / greatest value present; hi <= lo: identity; else in IEEE double, every operation
 *     rounded once: scale = 255.0 / (hi - lo), offset = -lo * scale, lut[i] = clamp((int)(i * scale + offset), 0, 255), truncated.
 *   EQUALIZE, per channel with histogram h: nz the non-zero counts; fewer than two: identity; step = (sum(nz) - nz[last]) / 255;
 *     step == 0: identity; else acc = step / 2; for i = 0..255: lut[i] = min(acc / step, 255), then acc += h[i].
 * Only images whose output has three channels take a non-empty program (RGB / YCbCr sources, or any source under
 * JPGPU_BATCH_RGB_OUTPUT): another one is JPGPU_ERR_UNSUPPORTED.  A program is refused (jpgpu_colour_check: JPGPU_ERR_FORMAT) for
 * n > 4, an unknown operation, a factor that is not finite, negative or above 256, a SOLARIZE value that is no integer in 0..256, a
 * POSTERIZE value that is no integer in 1..8, a HUE value that is no integer in 0..255.
 * Operations from 16 on are not tables; both equal Pillow byte for byte:
 *    16 HUE           shift n      (h, s, v) = rgb2hsv(px); h = (h + n) & 255; hsv2rgb        P.convert("HSV"), h + n, .convert("RGB"):
 *                                  n an integer 0..255; n = 0 is the lossy round trip          torchvision's adjust_hue on a PIL image
 *    17 SHARPNESS     factor f     blend(SMOOTH(P), p, f) per channel value                   ImageEnhance.Sharpness(P).enhance(f)
 *   rgb2hsv / hsv2rgb: Pillow's (Convert.c), float32 and double arithmetic with every operation rounded once, IEEE divisions.
 *   SMOOTH: the 3 x 3 filter (1 1 1, 1 5 1, 1 1 1) / 13 in float32 — 0.5f, then the three rows from the one below upwards, each
 *     (left k + middle k') + right k — truncated; the outermost row and column of every side are copied (W < 3 or H < 3: P itself).
 * `colour` NULL IS jpgpu_batch_create_oriented: same kernels, launches, bytes and path.  Otherwise every image starts with the empty
 * program; the batch's resample launch is the u8 one of the same arguments and writes the arena a warp reads, one launch behind it
 * (a workgroup per image) runs the programs there in place, and the batch's warp launch — with identity matrices in a batch without
 * warp options — writes the output arena.  jpgpu_batch_path gains "+colour" in front of "+warp..." / "+tensor".  Colour without an
 * output size: JPGPU_ERR_UNSUPPORTED, as RGB output; reserved != 0: JPGPU_ERR_FORMAT. */
enum {
    JPGPU_COLOUR_IDENTITY = 0, JPGPU_COLOUR_BRIGHTNESS = 1, JPGPU_COLOUR_CONTRAST = 2, JPGPU_COLOUR_COLOR = 3, JPGPU_COLOUR_SOLARIZE = 4,
    JPGPU_COLOUR_POSTERIZE = 5, JPGPU_COLOUR_INVERT = 6, JPGPU_COLOUR_AUTOCONTRAST = 7, JPGPU_COLOUR_EQUALIZE = 8,
    /* operations from 16 on are not tables (below); ids 9..15 and from 18 on are refused */
    JPGPU_COLOUR_HUE = 16, JPGPU_COLOUR_SHARPNESS = 17
};
typedef struct jpgpu_colour_op {
    uint32_t op; /* JPGPU_COLOUR_* */
    float value;
} jpgpu_colour_op;
typedef struct jpgpu_colour_program {
    uint32_t n; /* 0..4 */
    jpgpu_colour_op ops[4];
} jpgpu_colour_program;
typedef struct jpgpu_colour_options {
    uint32_t reserved; /* 0 */
} jpgpu_colour_options;
int jpgpu_batch_create_coloured(int device, const jpgpu_image_desc *descs, const jpgpu_window *windows, const jpgpu_placement *placements,
                                const uint8_t *fill, uint16_t out_w, uint16_t out_h, const jpgpu_tensor_format *format,
                                const jpgpu_warp_options *warp, const uint8_t *orientations, const jpgpu_colour_options *colour, uint32_t n_images,
                                uint32_t flags, jpgpu_batch **out);
/* The program of every image (`programs`: n_images entries; NULL: empty programs) from the next jpgpu_batch_decode enqueued on: built
 * into the images' job records, sent with them on the decode's stream (a decode already enqueued keeps its programs).  One refused
 * program refuses the call — JPGPU_ERR_FORMAT, or JPGPU_ERR_UNSUPPORTED for a non-empty program on an image without three output
 * channels — and nothing is changed.  JPGPU_ERR_UNSUPPORTED on a batch without colour. */
int jpgpu_batch_set_colour_programs(jpgpu_batch *b, const jpgpu_colour_program *programs);
/* Pure host functions (no device needed; the device runs the same bodies).  jpgpu_colour_check: the refusal rule above (JPGPU_OK /
 * JPGPU_ERR_FORMAT).  jpgpu_colour_point_lut: the 256-entry table of BRIGHTNESS, CONTRAST (with the image's mean `mean`, 0..255),
 * SOLARIZE, POSTERIZE, INVERT or IDENTITY; another operation or a refused value: JPGPU_ERR_FORMAT.  jpgpu_colour_autocontrast_lut /
 * jpgpu_colour_equalize_lut: one channel's table from its histogram h[256]. */
int jpgpu_colour_check(const jpgpu_colour_program *program);
int jpgpu_colour_point_lut(uint32_t op, float value, uint32_t mean, uint8_t *lut);
int jpgpu_colour_autocontrast_lut(const uint32_t *h, uint8_t *lut);
int jpgpu_colour_equalize_lut(const uint32_t *h, uint8_t *lut);
/* Programs on a caller's pixels: d_pixels holds n images of h x w x 3 bytes on the current device, one behind the other, and image i
 * goes through programs[i] in place, by the launch a coloured batch makes (`hip_stream`: a hipStream_t; NULL = the null stream).  The
 * call returns when the work is complete.  The programs are checked first: one refused program refuses the call, JPGPU_ERR_FORMAT,
 * and nothing is written.  d_pixels must be 256-byte aligned, 3 w h a multiple of 4, w and h 1..2048: else JPGPU_ERR_UNSUPPORTED. */
int jpgpu_colour_apply(uint8_t *d_pixels, uint32_t n, uint32_t w, uint32_t h, const jpgpu_colour_program *programs, void *hip_stream);
void jpgpu_batch_destroy(jpgpu_batch *b);
const char *jpgpu_batch_last_error(const jpgpu_batch *b);

/* Arena layout (bytes): coefficients of image i, component c start at coef_offset(i,c) and
 * hold block_w*block_h*64 int16 in block-raster order (the concatenation of that
 * component's append_row buffers); pixels of image i start at out_offset(i). */
size_t jpgpu_batch_coef_arena_bytes(const jpgpu_batch *b);
size_t jpgpu_batch_out_arena_bytes(const jpgpu_batch *b);
size_t jpgpu_batch_coef_offset(const jpgpu_batch *b, uint32_t image, uint32_t comp);
size_t jpgpu_batch_coef_bytes(const jpgpu_batch *b, uint32_t image, uint32_t comp);
size_t jpgpu_batch_out_offset(const jpgpu_batch *b, uint32_t image);
size_t jpgpu_batch_out_bytes(const jpgpu_batch *b, uint32_t image);

/* EXTERNAL_BUFFERS: device pointers owned by the caller (>= *_arena_bytes, 256-B aligned). */
int jpgpu_batch_bind(jpgpu_batch *b, void *device_coef_arena, void *device_out_arena);
void *jpgpu_batch_coef_arena(const jpgpu_batch *b); /* device pointer */
void *jpgpu_batch_out_arena(const jpgpu_batch *b);  /* device pointer */

/* Host -> HBM upload of one component's coefficients (also range-scans them, see
 * jpgpu_batch_set_range_hint). Blocking. */
int jpgpu_batch_upload(jpgpu_batch *b, uint32_t image, uint32_t comp, const int16_t *coefficients,
                       size_t len);
/* For coefficients written straight into a bound arena: range class of this image's
 * dequantized coefficients s = coefficient * q (what jpgpu_batch_upload computes itself):
 *   0  unknown / hostile -> wrap-exact kernels (always correct);
 *   1  every |s| < 2^15;
 *   3  additionally, in every 8x8 block, each column's sum of |s| is <= 5900.
 * Higher classes select faster arithmetic that is bit-exact only on such data.
 * Default for never-uploaded images: 0. */
int jpgpu_batch_set_range_hint(jpgpu_batch *b, uint32_t image, int sane);
/* Same, for one component; and the class of a buffer as jpgpu_batch_upload would compute it (pure host function,
 * no device needed) — for feeders that stage coefficients themselves (jpgpu_pipeline_*, jpgpu_decoder.h). */
int jpgpu_batch_set_range_class(jpgpu_batch *b, uint32_t image, uint32_t comp, int range_class);
int jpgpu_range_class(const int16_t *coefficients, size_t len, const uint16_t quantization_table[64]);
/* The same classification done ON THE DEVICE for every image of the batch, from the coefficients as they stand in the
 * arena (written there by the caller's own kernels or copies into a bound arena, or by the device entropy decoder; compact
 * uploads still waiting for a decode are expanded into it first, here and in jpgpu_batch_classify_on_device):
 * one pass over the arena at HBM speed on `hip_stream`, blocking; afterwards every component has the range class
 * jpgpu_batch_upload would have given it. If `classes` is not NULL it receives 4 entries per image. */
int jpgpu_batch_scan_ranges(jpgpu_batch *b, void *hip_stream, uint8_t *classes);
/* The classification WITHOUT the host: one pass over the arena on `hip_stream` (asynchronous, nothing is read back) leaves
 * per-image range statistics on the device, and from then on every jpgpu_batch_decode turns them into the images' classes
 * there (a few-microsecond kernel in front of the pixel kernels, which pick their arithmetic per workgroup) — no host
 * synchronisation between whoever wrote the coefficients and the pixel kernels.  The library's own writers leave the same
 * statistics as a by-product and need no pass at all: the device entropy decoder (jpgpu_pipeline_decode with
 * JPGPU_PIPELINE_DEVICE_ENTROPY), jpgpu_batch_upload_compact with range_class < 0.  A class set from
 * the host afterwards (upload, set_range_hint / set_range_class, scan_ranges) takes over again for that component. */
int jpgpu_batch_classify_on_device(jpgpu_batch *b, void *hip_stream);
/* Replace the quantization table given in the image descriptor (RowData.quantization_table of Worker::start,
 * src/worker/mod.rs:18-22): feeders learn it only while parsing the stream. Takes effect at the next decode enqueued (a decode
 * already enqueued keeps the old table: jpgpu_batch_decode).  If the table
 * differs from the one in place, the component's range class goes back to 0 (unknown: wrap-exact kernels) — the class of
 * coefficients uploaded earlier was computed with the old table; upload (or jpgpu_batch_set_range_class / scan_ranges) afterwards. */
int jpgpu_batch_set_quantization_table(jpgpu_batch *b, uint32_t image, uint32_t comp, const uint16_t quantization_table[64]);

/* Compact coefficient transport: PCIe carries, per component,
 *     [ n_blocks x u64 bitmap | n_blocks x u32 first-value index | nnz x i16 values ]
 * (bit k of a bitmap = natural-order coefficient k of the block is non-zero; values in ascending k; the index is the
 * block's position in the value array) and a kernel expands it into the coefficient arena at the start of the next
 * decode.  jpgpu_compact_encode converts `n_blocks` dense blocks (pure host function), returns the bytes written
 * (<= jpgpu_compact_max_bytes) and, if asked, the range class of jpgpu_batch_set_range_hint.
 * jpgpu_batch_upload_compact validates the buffer, copies it asynchronously on `hip_stream` (the buffer must stay
 * valid until that stream reaches the copy; use pinned memory for real overlap) and marks the component for expansion;
 * it also sets the component's range class when `range_class` >= 0; with `range_class` < 0 (the sender did not classify)
 * the expansion kernel ranges the values on the device while it has them in registers (jpgpu_batch_classify_on_device). */
size_t jpgpu_compact_max_bytes(size_t n_blocks);
size_t jpgpu_compact_encode(const int16_t *coefficients, size_t n_blocks, const uint16_t quantization_table[64], void *dst,
                            int *range_class);
int jpgpu_batch_upload_compact(jpgpu_batch *b, uint32_t image, uint32_t comp, const void *compact, size_t bytes,
                               int range_class, void *hip_stream);

/* Enqueue the whole batch on `hip_stream` (a hipStream_t; NULL = the null stream) and return: the decode is asynchronous.
 *
 * Batch calls on caller streams.  Every batch call that changes what a decode reads may be called as soon as jpgpu_batch_decode has
 * returned, whatever kind of stream the decode is queued on (blocking or hipStreamNonBlocking) and however much work lies in front
 * of it there: it affects only decodes enqueued LATER, the one already enqueued runs with the tables, classes, coefficients, arenas
 * and flips the batch held when it was enqueued.  This covers jpgpu_batch_set_quantization_table ("the next decode" below means the
 * next one enqueued), jpgpu_batch_set_range_hint, jpgpu_batch_set_range_class, jpgpu_batch_upload, jpgpu_batch_upload_compact,
 * jpgpu_batch_bind, jpgpu_batch_set_flips, jpgpu_batch_set_warps, jpgpu_batch_scan_ranges, jpgpu_batch_classify_on_device, and the decode that follows any
 * of them.  The library orders its own copies: where a table can only be rewritten by a blocking copy, the call that rewrites it
 * (jpgpu_batch_upload; the next decode, scan or classification after the others) first waits on the host for the work the batch
 * has enqueued — only when something did change, so a decode behind a decode gains no synchronisation.
 * Out of contract (the caller orders these itself):
 *   - decodes of one batch on two different streams without an event or a synchronisation between them;
 *   - a jpgpu_batch_upload_compact on another stream than the one the next decode uses;
 *   - the contents of the caller's own arenas under JPGPU_BATCH_EXTERNAL_BUFFERS (coefficients the caller writes into a bound arena,
 *     pixels it reads from one): the library orders its tables, not the caller's kernels and copies. */
int jpgpu_batch_decode(jpgpu_batch *b, void *hip_stream);
int jpgpu_batch_synchronize(jpgpu_batch *b, void *hip_stream);
/* HBM -> host download of one image's pixels. Blocking. */
int jpgpu_batch_download(jpgpu_batch *b, uint32_t image, uint8_t *dst, size_t cap, size_t *len);
/* Timing helper: `iters` back-to-back jpgpu_batch_decode on `hip_stream` bracketed by
 * hipEvents on that stream; returns the average milliseconds per decode of the batch. */
int jpgpu_batch_time(jpgpu_batch *b, void *hip_stream, uint32_t iters, float *ms_per_decode);
/* Name of the kernel path the batch resolved to ("fused420", "generic", ...). */
const char *jpgpu_batch_path(const jpgpu_batch *b);
/* How many images of the batch's fused launch groups run in each arithmetic variant (counts[0]: wrap-exact, counts[1]:
 * range class 1, counts[2]: range class 3) with the range classes as they stand: images of different classes get
 * separate launches, so an image with hostile coefficients costs only itself. Images on the generic path are not
 * counted (they carry their class per component). */
int jpgpu_batch_class_counts(jpgpu_batch *b, uint32_t counts[3]);

#ifdef __cplusplus
}
#endif
#endif /* JPGPU_H */
