"""A fixed output size (jpgpu_batch_create_resized, csrc/resample_band.hpp) on the MI355X.  The expected value is always
tests/resample_ref.py (the numpy statement of DESIGN.md §4.10, pinned to Pillow by tests/golden/resample) applied to the oracle's
whole decode sliced, compared with np.array_equal.  Batch first (coefficients in), then Pipeline (JPEG bytes in: the files, routes,
layouts and scales of tests/test_gpu_pipeline_windows.py)."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import oracle as O
import resample_ref as R
import synth
import test_gpu_pipeline_windows as PW
from test_window_emulation import grid_of, window_slice

pytestmark = pytest.mark.gpu

J = None


@pytest.fixture(scope="module", autouse=True)
def _load():
    global J
    import jpeg_decoder_amd as pkg
    J = pkg
    PW.J = pkg  # (its file makers use the package too)
    assert J.device_count() >= 1, "no MI355X visible: the HIP path has no CPU fallback"


def to_j(comps):
    out = (J.Component * len(comps))()
    for i, c in enumerate(comps):
        out[i].identifier, out[i].horizontal_sampling_factor, out[i].vertical_sampling_factor = c.identifier, c.h, c.v
        out[i].quantization_table_index, out[i].dct_scale = c.tq, c.dct_scale
        out[i].size_width, out[i].size_height, out[i].block_width, out[i].block_height = c.size_w, c.size_h, c.block_w, c.block_h
    return out


def _case(rng, w_, h_, samp, ct, scale=8, kind="sparse"):
    ocomps, _ = O.make_components(w_, h_, samp, dct_scale=scale)
    if kind == "sparse":
        qts = [rng.integers(1, 64, 64).astype(np.uint16) for _ in ocomps]
        coefs = [synth.sparse_coefficients(rng, c.block_w * c.block_h, amp=64, dc_amp=500) for c in ocomps]
    else:
        qts = [rng.integers(1, 65536, 64).astype(np.uint16) for _ in ocomps]
        coefs = [rng.integers(-32768, 32768, c.block_w * c.block_h * 64).astype(np.int16) for c in ocomps]
    ow, oh = J.scaled_output_size(w_, h_, scale)
    return ocomps, qts, coefs, ct, ow, oh


def _full(case):
    oc, qts, coefs, ct, ow, oh = case
    return O.pixels_from_coefficients(oc, qts, coefs, ow, oh, ct.upper())


def _desc(case):
    oc, qts, _c, ct, ow, oh = case
    return J.image_desc(list(to_j(oc)), qts, ow, oh, ct)


def source_of(case, full, win):
    """What the image gives without an output size, as (h, w, nc): its window, or its whole output."""
    oc, _q, _c, ct, ow, oh = case
    W, H = grid_of(oc, ow, oh)
    nc = len(oc)
    if win is None or win[2] == 0 or win[3] == 0:
        win = (0, 0, W, H)
    return window_slice(full, W, H, nc, ct, win).reshape(win[3], win[2], nc)


def want_resized(case, full, win, size):
    return R.resize(source_of(case, full, win), size[0], size[1]).reshape(-1)


def _upload(b, cases):
    for i, (oc, _q, coefs, *_r) in enumerate(cases):
        for c in range(len(oc)):
            b.upload(i, c, coefs[c])


def _decode(cases, windows, size, flags=0):
    b = J.Batch([_desc(c) for c in cases], flags=flags, windows=windows, output_size=size)
    try:
        _upload(b, cases)
        b.decode()
        b.synchronize()
        if size is not None:
            for i, case in enumerate(cases):
                assert b.out_bytes(i) == size[0] * size[1] * len(case[0])
        return [b.download(i) for i in range(len(cases))], b.path
    finally:
        b.close()


def _check(outs, cases, wins, fulls, size):
    for i, (case, full) in enumerate(zip(cases, fulls)):
        win = None if wins is None else wins[i]
        want = want_resized(case, full, win, size)
        assert outs[i].size == want.size, (i, outs[i].size, want.size)
        assert np.array_equal(outs[i], want), (i, case[4], case[5], win, size, np.nonzero(outs[i] != want)[0][:10].tolist())


# every interleaving colour function and every layout of tests/golden's families: 4:2:0, 4:4:4, 4:2:2, gray, CMYK / YCCK, RGB
LAYOUTS = [([(2, 2), (1, 1), (1, 1)], "YCbCr"), ([(1, 1), (1, 1), (1, 1)], "YCbCr"), ([(2, 1), (1, 1), (1, 1)], "YCbCr"), ([(1, 1)], "Grayscale"),
           ([(1, 1)] * 4, "CMYK"), ([(2, 2), (1, 1), (1, 1), (2, 2)], "YCCK"), ([(1, 1)] * 3, "RGB"), ([(4, 1), (1, 1), (1, 1)], "YCbCr")]
SIZES = [(1, 1), (17, 9), (161, 97), (50, 34), (640, 480), (24, 1100)]
OUT_SIZES = [(224, 224), (1, 1), (2048, 3), (37, 53)]


def _windows(W, H, k):
    """None, the whole image, odd interior windows, 1 x 1, windows at the right / bottom edges."""
    cand = [None, (0, 0, W, H), (W // 5 | 1, H // 7 | 1, max(1, (W // 2) | 1), max(1, (H // 2) | 1)), (W - 1, H - 1, 1, 1),
            (W // 3, 0, W - W // 3, max(1, H // 3)), (1, 1, max(1, W - 2), max(1, H - 2))]
    out = []
    for w in cand:
        if w is None or (w[0] + w[2] <= W and w[1] + w[3] <= H and w[2] > 0 and w[3] > 0):
            out.append(w)
    return out[k % len(out)], out[(k + 2) % len(out)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{'_'.join(f'{h}{v}' for h, v in l[0])}-{l[1]}")
@pytest.mark.parametrize("scale", [8, 4, 2, 1])
def test_batch_resize_bit_exact(layout, scale):
    """One batch per layout, scale and output size: every size with and without windows (odd ones included), in one launch."""
    samp, ct = layout
    rng = np.random.default_rng(scale * 1000 + len(samp) * 10 + len(ct))
    cases, wins, fulls = [], [], []
    for k, (w_, h_) in enumerate(SIZES):
        case = _case(rng, w_, h_, samp, ct, scale, "hostile" if k == 2 else "sparse")
        try:
            full = _full(case)
        except O.OracleError:  # (the reference refuses this frame: nothing to resample)
            continue
        oc, *_r, ow, oh = case
        W, H = grid_of(oc, ow, oh)
        for win in _windows(W, H, k + scale):
            cases.append(case), wins.append(win), fulls.append(full)
    assert len(cases) >= 8
    for size in OUT_SIZES:
        outs, path = _decode(cases, wins, size)
        assert path.endswith("+resize"), path
        _check(outs, cases, wins, fulls, size)


def test_batch_resize_without_windows_keeps_the_routes():
    """windows = NULL: every image's whole output resampled; the fused / scaled / generic routes only write somewhere else."""
    rng = np.random.default_rng(77)
    cases = [_case(rng, 640, 480, [(2, 2), (1, 1), (1, 1)], "YCbCr"), _case(rng, 333, 21, [(1, 1)] * 3, "RGB"),
             _case(rng, 250, 130, [(2, 2), (1, 1), (1, 1)], "YCbCr", 4), _case(rng, 64, 64, [(3, 1), (1, 1), (1, 1)], "YCbCr"),
             _case(rng, 300, 200, [(1, 1)], "Grayscale"), _case(rng, 640, 480, [(2, 2), (1, 1), (1, 1)], "YCbCr", kind="hostile")]
    fulls = [_full(c) for c in cases]
    plain, path0 = _decode(cases, None, None)
    outs, path = _decode(cases, None, (224, 224))
    assert path == path0 + "+resize" == "mixed+resize"
    _check(outs, cases, None, fulls, (224, 224))
    for a, f in zip(plain, fulls):
        assert np.array_equal(a, f)
    only420, p = _decode(cases[:1], None, (224, 224))
    assert p == "fused420+resize"
    assert np.array_equal(only420[0], outs[0])
    forced, p = _decode(cases, None, (224, 224), flags=J._native.BATCH_FORCE_GENERIC)
    assert p == "generic+resize"
    _check(forced, cases, None, fulls, (224, 224))


def test_batch_resize_equal_to_the_window_is_the_window():
    """An output size equal to every image's window: the identity under the rules, byte for byte the windowed decode."""
    rng = np.random.default_rng(3)
    cases = [_case(rng, 640, 480, [(2, 2), (1, 1), (1, 1)], "YCbCr"), _case(rng, 300, 250, [(1, 1)], "Grayscale"),
             _case(rng, 333, 240, [(1, 1)] * 4, "CMYK"), _case(rng, 227, 225, [(2, 1), (1, 1), (1, 1)], "YCbCr")]
    wins = [(101, 53, 227, 225), (73, 25, 227, 225), (1, 3, 227, 225), None]
    windowed, _p = _decode(cases, wins, None)
    outs, path = _decode(cases, wins, (227, 225))
    assert path == "mixed+resize"
    for a, b_ in zip(windowed, outs):
        assert np.array_equal(a, b_)
    _check(outs, cases, wins, [_full(c) for c in cases], (227, 225))


def test_batch_resize_upscaling_from_a_1x1_window():
    rng = np.random.default_rng(9)
    cases = [_case(rng, 161, 97, [(2, 2), (1, 1), (1, 1)], "YCbCr"), _case(rng, 50, 34, [(1, 1)], "Grayscale"), _case(rng, 1, 1, [(1, 1)] * 3, "RGB")]
    wins = [(77, 31, 1, 1), (49, 33, 1, 1), None]
    fulls = [_full(c) for c in cases]
    for size in [(224, 224), (2048, 512), (3, 1)]:
        outs, _p = _decode(cases, wins, size)
        _check(outs, cases, wins, fulls, size)
        for i, o in enumerate(outs):  # (one source pixel: every output pixel is that pixel)
            nc = len(cases[i][0])
            assert (o.reshape(-1, nc) == source_of(cases[i], fulls[i], wins[i]).reshape(1, nc)).all()


def test_batch_resize_2160p_to_224():
    rng = np.random.default_rng(2160)
    cases = [_case(rng, 3840, 2160, [(2, 2), (1, 1), (1, 1)], "YCbCr"), _case(rng, 3840, 2160, [(1, 1)], "Grayscale")]
    fulls = [_full(c) for c in cases]
    wins = [None, (1001, 3, 2839, 2157)]
    outs, path = _decode(cases, wins, (224, 224))
    assert path == "mixed+resize"
    _check(outs, cases, wins, fulls, (224, 224))


def test_batch_resize_chunked_vertical_path():
    """Output rows whose support does not fit the workgroup's LDS: the vertical sums gathered over chunks of source rows — a tall image
    to one or three rows, 1, 3 and 4 channels, widest rows."""
    rng = np.random.default_rng(12)
    cases = [_case(rng, 16, 1200, [(1, 1)] * 4, "CMYK"), _case(rng, 40, 3000, [(1, 1)], "Grayscale"), _case(rng, 24, 2000, [(1, 1)] * 3, "RGB"),
             _case(rng, 24, 2000, [(2, 2), (1, 1), (1, 1)], "YCbCr")]
    wins = [None, (3, 1, 31, 2998), None, (1, 7, 22, 1990)]
    fulls = [_full(c) for c in cases]
    for size in [(2048, 1), (2048, 3), (2047, 2), (333, 1)]:
        outs, _p = _decode(cases, wins, size)
        _check(outs, cases, wins, fulls, size)


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


@pytest.mark.parametrize("size", [(224, 224), (37, 53), (1, 1), (2048, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_batch_resize_arena_canary(size):
    """A caller's output arena poisoned beforehand: every byte of every resized image is written, no byte between images changes."""
    hip = _hip()
    rng = np.random.default_rng(300 + size[0])
    layouts = [([(2, 2), (1, 1), (1, 1)], "YCbCr"), ([(1, 1)] * 3, "RGB"), ([(2, 1), (1, 1), (1, 1)], "YCbCr"), ([(1, 1)], "Grayscale"),
               ([(2, 2), (1, 1), (1, 1), (2, 2)], "YCCK"), ([(4, 1), (1, 1), (1, 1)], "YCbCr")]
    sizes = [(250, 130), (1930, 40), (33, 17), (640, 480), (9, 300), (64, 48)]
    cases = [_case(rng, w_, h_, samp, ct) for (samp, ct), (w_, h_) in zip(layouts, sizes)]
    wins = []
    for k, case in enumerate(cases):
        oc, *_r, ow, oh = case
        W, H = grid_of(oc, ow, oh)
        w, h = max(1, W // 2 + 1), max(1, H // 3 + 1)
        wins.append((min(W - w, W // 5 + 1), min(H - h, H // 4), w, h) if k % 3 else None)
    fulls = [_full(c) for c in cases]
    b = J.Batch([_desc(c) for c in cases], flags=J._native.BATCH_EXTERNAL_BUFFERS, windows=wins, output_size=size)
    coef, out = C.c_void_p(), C.c_void_p()
    nco, nout = b.coef_arena_bytes(), b.out_arena_bytes()
    assert hip.hipMalloc(C.byref(coef), nco) == 0 and hip.hipMalloc(C.byref(out), nout + 4096) == 0
    try:
        b.bind(coef.value, out.value)
        _upload(b, cases)
        for pattern in (0xA5, 0x3C):
            assert hip.hipMemset(out, pattern, nout + 4096) == 0
            b.decode()
            b.synchronize()
            host = np.empty(nout + 4096, np.uint8)
            assert hip.hipMemcpy(host.ctypes.data, out, nout + 4096, 2) == 0
            covered = np.zeros(nout + 4096, bool)
            for i, (case, win) in enumerate(zip(cases, wins)):
                want = want_resized(case, fulls[i], win, size)
                off = b.out_offset(i)
                assert b.out_bytes(i) == want.size == size[0] * size[1] * len(case[0])
                assert np.array_equal(host[off: off + want.size], want), (size, hex(pattern), i, win)
                covered[off: off + want.size] = True
            assert (host[~covered] == pattern).all(), "the resample kernel wrote outside the images"
    finally:
        b.close()
        hip.hipFree(coef)
        hip.hipFree(out)


def test_batch_resize_refusals():
    """Each fails its creation alone: a size of 0 or above 2048 (FormatError), planar output (UnsupportedError), a window outside."""
    rng = np.random.default_rng(1)
    case = _case(rng, 64, 48, [(2, 2), (1, 1), (1, 1)], "YCbCr")
    for size in [(0, 0), (0, 224), (224, 0), (2049, 224), (224, 2049), (65535, 1)]:
        with pytest.raises(J.FormatError, match="output size"):
            J.Batch([_desc(case)], output_size=size)
    J.Batch([_desc(case)], output_size=(2048, 2048)).close()
    for samp in ([(1, 1)] * 3, [(1, 1)] * 4):
        planar = _case(rng, 64, 48, samp, "None")
        J.Batch([_desc(planar)], windows=[(1, 1, 9, 9)]).close()  # (without an output size it decodes)
        with pytest.raises(J.UnsupportedError, match="planar"):
            J.Batch([_desc(planar)], output_size=(8, 8))
        with pytest.raises(J.UnsupportedError, match="planar"):
            J.Batch([_desc(case), _desc(planar)], windows=[None, (1, 1, 9, 9)], output_size=(8, 8))
    gray_none = _case(rng, 64, 48, [(1, 1)], "None")  # (one component is never planar)
    outs, _p = _decode([gray_none], None, (8, 8))
    _check(outs, [gray_none], None, [_full(gray_none)], (8, 8))
    with pytest.raises(J.FormatError, match="outside"):
        J.Batch([_desc(case)], windows=[(60, 0, 5, 1)], output_size=(8, 8))


def test_batch_without_an_output_size_is_what_it_was():
    """No output size: the same paths and bytes, the arena holds the windows' / whole images' bytes."""
    rng = np.random.default_rng(21)
    cases = [_case(rng, 640, 480, [(2, 2), (1, 1), (1, 1)], "YCbCr"), _case(rng, 300, 200, [(1, 1)], "Grayscale")]
    wins = [(100, 50, 333, 217), None]
    outs, path = _decode(cases, wins, None)
    assert path == "mixed"
    for o, case, win in zip(outs, cases, wins):
        assert np.array_equal(o, source_of(case, _full(case), win).reshape(-1))
    outs, path = _decode(cases, None, None)
    assert path == "mixed"
    b = J.Batch([_desc(c) for c in cases])
    assert b.output_size is None and b.out_bytes(0) == 640 * 480 * 3 and b.out_arena_bytes() == 640 * 480 * 3 + 60160
    b.close()


def test_batch_resize_decodes_again_after_new_coefficients():
    """A reused batch: other coefficients, the same tables — the intermediate arena is rewritten, then resampled."""
    rng = np.random.default_rng(8)
    a = _case(rng, 320, 240, [(2, 2), (1, 1), (1, 1)], "YCbCr")
    b2 = (a[0], a[1], [synth.sparse_coefficients(rng, c.block_w * c.block_h, amp=64, dc_amp=500) for c in a[0]], *a[3:])
    b = J.Batch([_desc(a)], windows=[(11, 7, 200, 150)], output_size=(64, 48))
    try:
        for case in (a, b2, a):
            _upload(b, [case])
            b.decode()
            b.synchronize()
            assert np.array_equal(b.download(0), want_resized(case, _full(case), (11, 7, 200, 150), (64, 48)))
    finally:
        b.close()


# ======================================================== Pipeline ========================================================================
def _p_source(data, scale, ct, win):
    full, W, H, nc = PW._want(data, scale, ct)
    eff = (0, 0, W, H) if (win is None or win[2] == 0 or win[3] == 0) else tuple(win)
    return PW._slice(full, W, H, nc, ct, win).reshape(eff[3], eff[2], nc), eff, (W, H, nc)


def _p_check(p, files, wins, out, size, scale=None, ct=None, label=""):
    """Every image of the call against resample_ref of the oracle's slice; window(i) and info(i) keep reporting the window and the
    image, the byte counts are the resized ones."""
    bad = []
    for i, data in enumerate(files):
        win = None if wins is None else wins[i]
        src, eff, (W, H, nc) = _p_source(data, scale, ct, win)
        want = R.resize(src, size[0], size[1]).reshape(-1)
        got = out[i]
        if isinstance(got, Exception):
            bad.append((i, win, repr(got)))
            continue
        if not np.array_equal(got, want):
            bad.append((i, win, (W, H, nc), got.size, want.size))
        assert p.window(i) == eff, (label, i, p.window(i), eff)
        assert J._native.lib().jpgpu_pipeline_pixel_bytes(p._h, i) == size[0] * size[1] * nc, (label, i)
        if nc > 1:
            assert (p.info(i).width, p.info(i).height) == (W, H), (label, i)
    assert not bad, (label, size, bad[:8], len(bad))


P_MATRIX = [m for m in PW.MATRIX if m[1] != "none"]  # (planar output is refused: test_pipeline_planar_images_fail_alone)


def test_pipeline_matrix_covers_every_route_layout_scale_and_size():
    assert {m[0] for m in P_MATRIX} == set(PW.ROUTES) and {m[1] for m in P_MATRIX} == set(PW.LAYOUTS) - {"none"}
    assert {m[2] for m in P_MATRIX} == set(PW.SCALES)
    assert {OUT_SIZES[k % len(OUT_SIZES)] for k in range(len(P_MATRIX))} == set(OUT_SIZES)
    for r in PW.ROUTES:  # (every route sees 224 x 224 and at least one other size)
        assert len({OUT_SIZES[k % len(OUT_SIZES)] for k, m in enumerate(P_MATRIX) if m[0] == r}) >= 2, r


@pytest.mark.parametrize("k", range(len(P_MATRIX)), ids=[f"{r}-{l}-s{s}" for r, l, s in P_MATRIX])
def test_pipeline_resize_matrix(monkeypatch, k):
    """One call per case: baseline, restart and progressive streams on the host and device entropy routes, every layout, with `scale=`,
    two image sizes, every window shape of windows_of() as an image of its own (odd ones, whole-image ones and None included)."""
    route, layout, s = P_MATRIX[k]
    size = OUT_SIZES[k % len(OUT_SIZES)]
    enc, kwargs, env = PW.ROUTES[route]
    flayout, ct, sizes = PW.LAYOUTS[layout]
    big = sizes[0]
    scale = None if s == 8 else (-(-big[0] * s // 8), -(-big[1] * s // 8))
    files, wins = [], []
    for j, sz in enumerate(sizes):
        data = PW._file(flayout, enc, sz, pic=j)
        _full, W, H, _nc = PW._want(data, scale, ct)
        for win in PW.windows_of(W, H):
            files.append(data), wins.append(win)
    PW._env(monkeypatch, env)
    p = J.Pipeline(threads=4)
    try:
        out = p.decode(files, scale=scale, color_transform=ct, windows=wins, output_size=size, **kwargs)
        t = p.timings()
        _p_check(p, files, wins, out, size, scale, ct, label=f"{route} {layout} s{s}")
        n_win = sum(1 for f, w in zip(files, wins) if w is not None and w != (0, 0) + PW._want(f, scale, ct)[1:3])
        assert t["images_resized"] == t["images_ok"] == len(files) and t["images_windowed"] == n_win, t
        assert t["pixel_bytes"] == sum(o.size for o in out), t
        assert p.kernel_path.endswith("+resize") or p.kernel_path == "mixed", p.kernel_path
        if layout in PW.BE.SAMPLINGS:  # (files of the encoders: the routes are known, and an output size changes none)
            if route in ("device", "device-restart", "host-staged"):
                assert t["images_device_entropy"] == len(files) and t["images_device_rejected"] == 0, t
            elif route == "prog-device":
                assert t["images_device_progressive"] == len(files) and t["images_device_rejected"] == 0, t
            else:
                assert t["images_device_entropy"] == 0, t
    finally:
        p.close()


def test_pipeline_planar_images_fail_alone(monkeypatch):
    PW._env(monkeypatch, {})
    planar, plain = PW._file("444", "base", (161, 97)), PW._file("420", "base", (161, 97), pic=1)
    gray = PW._file("gray", "base", (161, 97))
    p = J.Pipeline(threads=4)
    try:
        files = [planar, planar, gray]
        out = p.decode(files, color_transform="None", output_size=(32, 24), windows=[None, (5, 3, 7, 5), None])
        assert isinstance(out[0], J.UnsupportedError) and "planar" in str(out[0]), out[0]
        assert isinstance(out[1], J.UnsupportedError)
        src, eff, _g = _p_source(gray, None, "None", None)  # (one component is never planar)
        assert np.array_equal(out[2], R.resize(src, 32, 24).reshape(-1)) and p.window(2) == eff
        assert p.window(1) == (5, 3, 7, 5) and p.info(0).width == 161  # (the refused images' windows were fine: still reported)
        assert p.timings()["images_ok"] == 1 and p.timings()["images_resized"] == 1
        out = p.decode(files, color_transform="None", windows=[None, (5, 3, 7, 5), None])  # (without an output size they decode)
        PW._check_call(p, files, [None, (5, 3, 7, 5), None], out, None, "None")
        out = p.decode([planar, plain], output_size=(32, 24))  # (their own transform, YCbCr: interleaved)
        _p_check(p, [planar, plain], None, out, (32, 24))
    finally:
        p.close()


def test_pipeline_errors_are_per_image_and_bad_sizes_change_nothing(monkeypatch):
    PW._env(monkeypatch, {"JPGPU_PIPE_FORCE_DEVICE": "1"})
    good = PW._file("420", "base", (333, 200), pic=0)
    unreadable = b"\xff\xd8\xff\xe0\x00\x03"
    files = [good, good, unreadable, good]
    wins = [(300, 100, 40, 40), (100, 50, 80, 60), None, None]
    p = J.Pipeline(threads=4)
    try:
        out = p.decode(files, windows=wins, output_size=(224, 224))
        assert isinstance(out[0], J.FormatError) and "window" in str(out[0]), out[0]
        assert isinstance(out[2], Exception)
        for k in (1, 3):
            src, _e, _g = _p_source(files[k], None, None, wins[k])
            assert np.array_equal(out[k], R.resize(src, 224, 224).reshape(-1)), k
        assert p.window(0) is None and p.timings()["images_resized"] == 2
        for bad in [(0, 224), (224, 0), (2049, 224), (224, 2049)]:
            with pytest.raises(J.FormatError, match="output size"):
                p.decode(files, output_size=bad)
        lib = J._native.lib()  # (the refused size left the one before in force: sticky, like the scale)
        assert lib.jpgpu_pipeline_set_output_size(p._h, 3000, 5) == J._native.ERR_FORMAT
        ptrs = (C.c_char_p * 1)(good)
        lens = (C.c_size_t * 1)(len(good))
        assert lib.jpgpu_pipeline_set_output_size(p._h, 64, 48) == 0
        assert lib.jpgpu_pipeline_set_output_size(p._h, 0, 48) == J._native.ERR_FORMAT
        assert lib.jpgpu_pipeline_decode(p._h, C.cast(ptrs, C.POINTER(C.c_void_p)), lens, 1, J._native.PIPELINE_DOWNLOAD) == 0
        assert lib.jpgpu_pipeline_pixel_bytes(p._h, 0) == 64 * 48 * 3
        assert lib.jpgpu_pipeline_set_output_size(p._h, 0, 0) == 0
        assert lib.jpgpu_pipeline_decode(p._h, C.cast(ptrs, C.POINTER(C.c_void_p)), lens, 1, J._native.PIPELINE_DOWNLOAD) == 0
        assert lib.jpgpu_pipeline_pixel_bytes(p._h, 0) == 333 * 200 * 3
    finally:
        p.close()


def test_pipeline_resized_bytes_by_every_download_mode(monkeypatch):
    PW._env(monkeypatch, {})
    files = [PW._file("420", "base", (333, 200), pic=k) for k in range(6)] + [PW._file("gray", "base", (161, 97), pic=1)]
    wins = [(13, 5, 101, 77), None, (0, 0, 333, 200), (332, 199, 1, 1), (0, 7, 333, 1), (16, 16, 64, 32), (5, 3, 7, 5)]
    size = (224, 224)
    p = J.Pipeline(threads=4)
    try:
        a = p.decode(files, windows=wins, download=True, output_size=size)
        _p_check(p, files, wins, a, size, label="download=True")
        t = p.timings()
        assert t["pixel_bytes"] == sum(x.size for x in a) == 6 * 224 * 224 * 3 + 224 * 224, t
        counts = p.decode(files, windows=wins, download="pinned", output_size=size)
        assert counts == [x.size for x in a]
        b = [p.pixels_host(i).copy() for i in range(len(files))]
        counts = p.decode(files, windows=wins, download=False, output_size=size)
        assert counts == [x.size for x in a]
        assert p.pixels_host(0) is None
        c = [p.download(i) for i in range(len(files))]
        for i in range(len(files)):
            assert np.array_equal(a[i], b[i]) and np.array_equal(a[i], c[i]), i
            assert p.device_pointer(i)
    finally:
        p.close()


def test_pipeline_output_size_on_off_and_changed_between_calls(monkeypatch, capfd):
    """One pipeline, kept sub-batches: the output size switched on, changed, kept with fresh windows (set in place), switched off and on
    again.  Slot k of call c holds another picture than in call c - 1, so pixels left over from the call before cannot pass."""
    n = 64
    W, H = 333, 200
    steps = [(None, None), ((224, 224), "A"), ((224, 224), "B"), ((224, 224), "C"), ((64, 48), "C"), ((64, 48), None), (None, "A"), ((224, 224), "A"),
             ((224, 224), "B"), ((1, 1), "half"), (None, None), ((2048, 3), "B"), ((2048, 3), "A")]
    in_place = {2, 3, 8, 12}  # (the same output size and set of windowed images as the call before, other windows)
    p = J.Pipeline(threads=4)
    try:
        for c, (size, wname) in enumerate(steps):
            PW._env(monkeypatch, {})
            monkeypatch.setenv("JPGPU_PIPE_TRACE", "1")
            files = [PW._file("420", "base", (W, H), pic=(k + n // 2 * (c % 2)) % n) for k in range(n)]
            wins = PW._windows_set(wname, n)
            capfd.readouterr()
            out = p.decode(files, windows=wins, output_size=size)
            trace = capfd.readouterr().err
            t = p.timings()
            assert t["images_ok"] == n and t["images_device_rejected"] == 0 and t["images_device_entropy"] == n, (c, t)
            n_win = 0 if wins is None else sum(w is not None for w in wins)
            assert t["images_windowed"] == n_win and t["images_entry_pixels"] == n - n_win, (c, t)
            assert t["images_resized"] == (n if size else 0), (c, t)
            if size is None:  # what a pipeline without the feature gives: path, counters, bytes
                assert p.kernel_path == ("fused420" if n_win == 0 else ("window" if n_win == n else "mixed")), (c, p.kernel_path)
                assert t["pixel_bytes"] == sum(W * H * 3 if (wins is None or wins[k] is None) else wins[k][2] * wins[k][3] * 3 for k in range(n))
                PW._check_call(p, files, wins if wins else [None] * n, out, label=f"call {c}")
            else:
                assert p.kernel_path.endswith("+resize"), (c, p.kernel_path)
                assert t["pixel_bytes"] == n * size[0] * size[1] * 3
                _p_check(p, files, wins, out, size, label=f"call {c}")
            assert ("re-windowed in place" in trace) == (c in in_place), (c, trace[-600:])
            if c and steps[c - 1][0] != size:
                assert "created" in trace, (c, trace[-600:])
    finally:
        monkeypatch.delenv("JPGPU_PIPE_TRACE", raising=False)
        p.close()


@pytest.mark.parametrize("gather", [False, True], ids=["plain", "gather"])
def test_pipeline_resize_two_children_on_one_device(monkeypatch, gather):
    """One device listed twice: both children resample their share; with `gather` the gathered copy holds the resized bytes."""
    PW._env(monkeypatch, {})
    n = 96
    size = (37, 53)
    files = [PW._file("420", "base", (333, 200) if k % 3 else (161, 97), pic=k % 8) for k in range(n)]
    wins = [None if k % 5 == 0 else ((13 + k, 5 + k % 9, 41 + 2 * (k % 20), 33) if k % 3 else (5, 3, 7 + 2 * (k % 30), 5 + k % 40)) for k in range(n)]
    p = J.Pipeline(devices=[0, 0], threads=4)
    try:
        p.decode(files, windows=wins, gather=gather, download=False, output_size=size)
        t = p.timings()
        assert t["images_ok"] == t["images_resized"] == n and t["pixel_bytes"] == n * 37 * 53 * 3, t
        if gather:
            assert 0 < t["gather_bytes"] < n * (37 * 53 * 3 + 512) + 4096, t  # (the resized arenas travel, not the windows)
        got = [p.download(i) for i in range(n)]
        _p_check(p, files, wins, got, size, label="two children")
        if gather:
            hip = C.CDLL("libamdhip64.so")
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            for i in range(n):
                buf = np.empty(got[i].size, np.uint8)
                assert hip.hipMemcpy(buf.ctypes.data, p.device_pointer(i), buf.size, 2) == 0
                assert np.array_equal(buf, got[i]), i
        out = p.decode(files, windows=wins, gather=gather, output_size=size)
        _p_check(p, files, wins, out, size, label="two children, downloaded")
    finally:
        p.close()


def test_pipeline_1024_files_of_1080p_random_resized_crops_to_224(monkeypatch):
    """A loader's call: 1,024 files, a RandomResizedCrop window each, every image 224 x 224 x 3 in the pinned block — every image compared."""
    PW._env(monkeypatch, {})
    n, distinct = 1024, 8
    pics = [PW.BE.synthetic_jpeg(1920, 1080, seed=9000 + k) for k in range(distinct)]
    fulls = [O.decode(d).pixels.reshape(1080, 1920, 3) for d in pics]
    rng = np.random.default_rng(20261017)
    wins = PW.random_resized_crops(rng, n, 1920, 1080)
    assert any(w[0] % 2 and w[1] % 2 for w in wins)
    files = [pics[k % distinct] for k in range(n)]
    p = J.Pipeline()
    try:
        counts = p.decode(files, windows=wins, download="pinned", output_size=(224, 224))
        t = p.timings()
        assert t["images_ok"] == t["images_resized"] == n and t["images_device_rejected"] == 0, t
        assert t["pixel_bytes"] == n * 224 * 224 * 3
        assert counts == [224 * 224 * 3] * n
        got = [hashlib.sha256(p.pixels_host(i)).digest() for i in range(n)]
        bad = []
        for i, (x, y, w, h) in enumerate(wins):
            want = R.resize(fulls[i % distinct][y:y + h, x:x + w], 224, 224)
            if hashlib.sha256(np.ascontiguousarray(want)).digest() != got[i]:
                bad.append((i, wins[i]))
        assert not bad, (bad[:10], len(bad))
    finally:
        p.close()
