"""The tensor output (jpgpu_batch_create_tensor, csrc/tensor_band.hpp) on the MI355X.  The expected value is always
tests/tensor_ref.py of tests/resample_ref.py of the oracle's whole decode sliced, compared with np.array_equal on the bit patterns.
Batch first (coefficients in), then Pipeline (JPEG bytes in: the files and routes of tests/test_gpu_pipeline_windows.py)."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import oracle as O
import resample_ref as R
import tensor_ref as T
import test_gpu_pipeline_windows as PW
import test_gpu_resize as RZ
from test_window_emulation import grid_of

pytestmark = pytest.mark.gpu

J = None


@pytest.fixture(scope="module", autouse=True)
def _load():
    global J
    import jpeg_decoder_amd as pkg
    J = pkg
    PW.J = pkg
    RZ.J = pkg
    assert J.device_count() >= 1, "no MI355X visible: the HIP path has no CPU fallback"


FORMATS = {"float32": T.IMAGENET, "float16": T.CLIP, "bfloat16": T.HALF}


def fmt_of(dtype, which=None):
    mean, std = which or FORMATS[dtype]
    return J.TensorFormat(dtype, mean, std), (dtype, mean, std)


def want_tensor(case, full, win, size, ref_fmt, flip):
    src = RZ.source_of(case, full, win)
    return T.bits(T.to_tensor(R.resize(src, size[0], size[1]), T.table(ref_fmt, src.shape[2]), flip))


def _decode(cases, wins, size, fmt, flips, flags=0):
    b = J.Batch([RZ._desc(c) for c in cases], flags=flags, windows=wins, output_size=size, tensor=fmt)
    try:
        RZ._upload(b, cases)
        if flips is not None:
            b.set_flips(flips)
        b.decode()
        b.synchronize()
        for i, case in enumerate(cases):
            assert b.out_bytes(i) == size[0] * size[1] * len(case[0]) * fmt.itemsize
            assert b.out_offset(i) % 256 == 0
        return [b.download(i) for i in range(len(cases))], b.path
    finally:
        b.close()


def _check(outs, cases, wins, fulls, size, fmt, ref_fmt, flips):
    for i, (case, full) in enumerate(zip(cases, fulls)):
        win = None if wins is None else wins[i]
        flip = bool(flips[i]) if flips is not None else False
        want = want_tensor(case, full, win, size, ref_fmt, flip)
        assert outs[i].dtype == fmt.numpy_dtype and outs[i].shape == want.shape == (len(case[0]), size[1], size[0]), (i, outs[i].shape, want.shape)
        got = T.bits(outs[i])
        assert np.array_equal(got, want), (i, case[4], case[5], win, size, flip, np.argwhere(got != want)[:6].tolist())


# the eight layouts of tests/test_gpu_resize.py
LAYOUTS = [([(2, 2), (1, 1), (1, 1)], "YCbCr"), ([(1, 1), (1, 1), (1, 1)], "YCbCr"), ([(2, 1), (1, 1), (1, 1)], "YCbCr"), ([(1, 1)], "Grayscale"),
           ([(1, 1)] * 4, "CMYK"), ([(2, 2), (1, 1), (1, 1), (2, 2)], "YCCK"), ([(1, 1)] * 3, "RGB"), ([(4, 1), (1, 1), (1, 1)], "YCbCr")]
SIZES = [(1, 1), (17, 9), (161, 97), (50, 34), (640, 480)]
OUT_SIZES = [(224, 224), (1, 1), (37, 53), (2048, 3)]
_LAYOUT_CASES = {}


def _layout_cases(k):
    """The images of a layout with their windows and the oracle's decodes: made once, shared by the dtypes, never changed."""
    if k not in _LAYOUT_CASES:
        samp, ct = LAYOUTS[k]
        rng = np.random.default_rng(5000 + k)
        cases, wins, fulls = [], [], []
        for n, (w_, h_) in enumerate(SIZES):
            case = RZ._case(rng, w_, h_, samp, ct, 8, "hostile" if n == 2 else "sparse")
            full = RZ._full(case)
            oc, *_r, ow, oh = case
            W, H = grid_of(oc, ow, oh)
            for win in RZ._windows(W, H, n + k):
                cases.append(case), wins.append(win), fulls.append(full)
        _LAYOUT_CASES[k] = (cases, wins, fulls)
    return _LAYOUT_CASES[k]


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("k", range(len(LAYOUTS)), ids=[f"{'_'.join(f'{h}{v}' for h, v in l[0])}-{l[1]}" for l in LAYOUTS])
def test_batch_tensor_bit_exact(k, dtype):
    """One launch per layout, dtype and output size: every image size with windows (odd, 1 x 1, at the edges, none), every other image
    flipped."""
    cases, wins, fulls = _layout_cases(k)
    assert len(cases) >= 8
    fmt, ref_fmt = fmt_of(dtype)
    flips = [i % 2 == 1 for i in range(len(cases))]
    for size in OUT_SIZES:
        outs, path = _decode(cases, wins, size, fmt, flips)
        assert path.endswith("+resize+tensor"), path
        _check(outs, cases, wins, fulls, size, fmt, ref_fmt, flips)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_batch_tensor_chunked_vertical_path(dtype):
    """Output rows whose support does not fit the workgroup's LDS: the sums gathered over chunks of source rows, four-pixel items
    (2048 columns) and element items (333), flipped and not."""
    rng = np.random.default_rng(12)
    cases = [RZ._case(rng, 24, 2000, [(1, 1)] * 3, "RGB"), RZ._case(rng, 16, 1200, [(1, 1)] * 4, "CMYK")] * 2
    fulls = [RZ._full(c) for c in cases[:2]] * 2
    flips = [False, False, True, True]
    fmt, ref_fmt = fmt_of(dtype)
    for size in [(2048, 1), (333, 1)]:
        outs, _p = _decode(cases, None, size, fmt, flips)
        _check(outs, cases, None, fulls, size, fmt, ref_fmt, flips)


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("size", [(224, 224), (37, 53), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_batch_tensor_arena_canary(size, dtype):
    """A caller's output arena poisoned beforehand, two patterns: every element of every tensor is written, no byte between or behind
    the images changes."""
    hip = _hip()
    rng = np.random.default_rng(300 + size[0])
    layouts = [([(2, 2), (1, 1), (1, 1)], "YCbCr"), ([(1, 1)] * 3, "RGB"), ([(1, 1)], "Grayscale"), ([(2, 2), (1, 1), (1, 1), (2, 2)], "YCCK"), ([(1, 1)], "Grayscale")]
    sizes = [(250, 130), (33, 17), (640, 480), (9, 300), (64, 48)]
    cases = [RZ._case(rng, w_, h_, samp, ct) for (samp, ct), (w_, h_) in zip(layouts, sizes)]
    wins = [None, (3, 1, 29, 15), (101, 53, 333, 217), None, (1, 1, 61, 45)]
    flips = [True, False, True, True, False]
    fulls = [RZ._full(c) for c in cases]
    fmt, ref_fmt = fmt_of(dtype)
    b = J.Batch([RZ._desc(c) for c in cases], flags=J._native.BATCH_EXTERNAL_BUFFERS, windows=wins, output_size=size, tensor=fmt)
    coef, out = C.c_void_p(), C.c_void_p()
    nco, nout = b.coef_arena_bytes(), b.out_arena_bytes()
    assert hip.hipMalloc(C.byref(coef), nco) == 0 and hip.hipMalloc(C.byref(out), nout + 4096) == 0
    try:
        b.bind(coef.value, out.value)
        RZ._upload(b, cases)
        b.set_flips(flips)
        for pattern in (0xA5, 0x3C):
            assert hip.hipMemset(out, pattern, nout + 4096) == 0
            b.decode()
            b.synchronize()
            host = np.empty(nout + 4096, np.uint8)
            assert hip.hipMemcpy(host.ctypes.data, out, nout + 4096, 2) == 0
            covered = np.zeros(nout + 4096, bool)
            for i, (case, win) in enumerate(zip(cases, wins)):
                want = want_tensor(case, fulls[i], win, size, ref_fmt, flips[i])
                off = b.out_offset(i)
                assert b.out_bytes(i) == want.nbytes
                got = host[off: off + want.nbytes].view(want.dtype).reshape(want.shape)
                assert np.array_equal(got, want), (size, hex(pattern), i, win)
                covered[off: off + want.nbytes] = True
            assert (host[~covered] == pattern).all(), "the tensor kernel wrote outside the images"
    finally:
        b.close()
        hip.hipFree(coef)
        hip.hipFree(out)


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_batch_tensor_into_a_torch_tensor(dtype):
    """The user story: a torch.empty(N, 3, 224, 224) bound as the output arena IS the model's input.  Compared with torch's own
    conversion of the u8 batch's result, done on the CPU — the pinned arithmetic (on the device torch divides by a scalar through a
    multiplication with its reciprocal, which is another rounding)."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(44)
    n = 5
    cases = [RZ._case(rng, 320 + 16 * k, 240, [(2, 2), (1, 1), (1, 1)] if k % 2 else [(1, 1)] * 3, "YCbCr" if k % 2 else "RGB") for k in range(n)]
    wins = [None, (11, 7, 200, 150), (1, 1, 300, 200), None, (100, 100, 37, 41)]
    flips = [False, True, True, False, True]
    u8, _p = RZ._decode(cases, wins, (224, 224))
    fmt, _ref = fmt_of(dtype, T.IMAGENET)
    tdt = getattr(torch, dtype)
    x = torch.empty(n, 3, 224, 224, dtype=tdt, device="cuda")
    x.view(torch.int16 if fmt.itemsize == 2 else torch.int32).fill_(0x5A5A)
    b = J.Batch([RZ._desc(c) for c in cases], flags=J._native.BATCH_EXTERNAL_BUFFERS, windows=wins, output_size=(224, 224), tensor=fmt)
    try:
        assert b.out_arena_bytes() == x.numel() * x.element_size() and [b.out_offset(i) for i in range(n)] == [i * 3 * 224 * 224 * fmt.itemsize for i in range(n)]
        coef = torch.empty(b.coef_arena_bytes(), dtype=torch.uint8, device="cuda")
        b.bind(coef.data_ptr(), x.data_ptr())
        RZ._upload(b, cases)
        b.set_flips(flips)
        b.decode()
        b.synchronize()
    finally:
        b.close()
    mean = torch.tensor(T.IMAGENET[0][:3], dtype=torch.float32).view(1, 3, 1, 1)
    std = torch.tensor(T.IMAGENET[1][:3], dtype=torch.float32).view(1, 3, 1, 1)
    y = torch.from_numpy(np.stack(u8)).view(n, 224, 224, 3).permute(0, 3, 1, 2).to(torch.float32).div(255).sub(mean).div(std).to(tdt)
    y = torch.where(torch.tensor(flips).view(n, 1, 1, 1), y.flip(-1), y)
    it = torch.int16 if fmt.itemsize == 2 else torch.int32
    assert torch.equal(x.cpu().view(it), y.contiguous().view(it))


def test_batch_set_flips_between_decodes():
    """Flips take effect at the next decode, change the flipped images only, and NULL clears them; sizes and offsets never move."""
    rng = np.random.default_rng(8)
    cases = [RZ._case(rng, 161, 97, [(2, 2), (1, 1), (1, 1)], "YCbCr"), RZ._case(rng, 50, 34, [(1, 1)], "Grayscale"), RZ._case(rng, 64, 64, [(1, 1)] * 3, "RGB")]
    fulls = [RZ._full(c) for c in cases]
    wins = [(3, 5, 101, 77), None, None]
    size = (40, 24)
    fmt, ref_fmt = fmt_of("float16")
    b = J.Batch([RZ._desc(c) for c in cases], windows=wins, output_size=size, tensor=fmt)
    try:
        RZ._upload(b, cases)
        offs = [b.out_offset(i) for i in range(3)]
        for flips in (None, [True, False, False], [False, True, True], None, [True, True, True], [False] * 3):
            b.set_flips(flips)
            b.decode()
            b.synchronize()
            _check([b.download(i) for i in range(3)], cases, wins, fulls, size, fmt, ref_fmt, flips)
            assert offs == [b.out_offset(i) for i in range(3)]
        with pytest.raises(ValueError):
            b.set_flips([True])
    finally:
        b.close()


def test_batch_tensor_refusals():
    rng = np.random.default_rng(1)
    case = RZ._case(rng, 64, 48, [(2, 2), (1, 1), (1, 1)], "YCbCr")
    gray = RZ._case(rng, 64, 48, [(1, 1)], "Grayscale")
    fmt = J.TensorFormat("float32", *T.IMAGENET)
    with pytest.raises(J.FormatError, match="output size"):
        J.Batch([RZ._desc(case)], tensor=fmt)
    with pytest.raises(J.FormatError, match="output size"):
        J.Batch([RZ._desc(case)], tensor=fmt, output_size=(0, 8))
    for bad in (0.0, float("nan"), float("inf")):
        with pytest.raises(J.FormatError, match="std"):
            J.Batch([RZ._desc(case)], output_size=(8, 8), tensor=J.TensorFormat("float16", (0.5,) * 3, (0.5, 0.5, bad)))
        # (a channel no image of the call has is not looked at)
        J.Batch([RZ._desc(gray)], output_size=(8, 8), tensor=J.TensorFormat("float16", (0.5,) * 3, (0.5, 0.5, bad))).close()
        with pytest.raises(J.FormatError, match="std"):
            J.Batch([RZ._desc(gray), RZ._desc(case)], output_size=(8, 8), tensor=J.TensorFormat("float16", (0.5,) * 3, (0.5, 0.5, bad)))
    with pytest.raises(J.FormatError, match="mean"):
        J.Batch([RZ._desc(case)], output_size=(8, 8), tensor=J.TensorFormat("float32", (float("nan"), 0, 0)))
    planar = RZ._case(rng, 64, 48, [(1, 1)] * 3, "None")
    with pytest.raises(J.UnsupportedError, match="planar"):
        J.Batch([RZ._desc(case), RZ._desc(planar)], output_size=(8, 8), tensor=fmt)
    for kwargs in ({}, {"output_size": (8, 8)}, {"windows": [(1, 1, 9, 9)]}):  # (a batch of bytes has no flips)
        b = J.Batch([RZ._desc(case)], **kwargs)
        try:
            with pytest.raises(J.UnsupportedError, match="tensor"):
                b.set_flips([True])
        finally:
            b.close()


def test_batch_without_a_tensor_is_what_it_was():
    rng = np.random.default_rng(21)
    cases = [RZ._case(rng, 640, 480, [(2, 2), (1, 1), (1, 1)], "YCbCr"), RZ._case(rng, 300, 200, [(1, 1)], "Grayscale")]
    wins = [(100, 50, 333, 217), None]
    fulls = [RZ._full(c) for c in cases]
    outs, path = RZ._decode(cases, wins, (224, 224))
    assert path == "mixed+resize"
    RZ._check(outs, cases, wins, fulls, (224, 224))
    assert all(o.dtype == np.uint8 and o.ndim == 1 for o in outs)
    outs, path = RZ._decode(cases, wins, None)
    assert path == "mixed"
    for o, case, win, full in zip(outs, cases, wins, fulls):
        assert np.array_equal(o, RZ.source_of(case, full, win).reshape(-1))
    b = J.Batch([RZ._desc(c) for c in cases], output_size=(224, 224))
    assert b.tensor is None and b.out_bytes(0) == 224 * 224 * 3 and b.out_arena_bytes() == 224 * 224 * 3 + 224 * 224
    b.close()


def test_batch_tensor_2160p_to_224_f16():
    rng = np.random.default_rng(2160)
    cases = [RZ._case(rng, 3840, 2160, [(2, 2), (1, 1), (1, 1)], "YCbCr")]
    fulls = [RZ._full(c) for c in cases]
    fmt, ref_fmt = fmt_of("float16", T.IMAGENET)
    outs, path = _decode(cases, None, (224, 224), fmt, [True])
    assert path == "fused420+resize+tensor"
    _check(outs, cases, None, fulls, (224, 224), fmt, ref_fmt, [True])


# ======================================================== Pipeline ========================================================================
def _p_want(data, scale, ct, win, size, ref_fmt, flip):
    src, eff, geom = RZ._p_source(data, scale, ct, win)
    return T.bits(T.to_tensor(R.resize(src, size[0], size[1]), T.table(ref_fmt, src.shape[2]), flip)), eff, geom


def _p_check(p, files, wins, flips, out, size, fmt, ref_fmt, scale=None, ct=None, label=""):
    bad = []
    for i, data in enumerate(files):
        win = None if wins is None else wins[i]
        flip = bool(flips[i]) if flips is not None else False
        want, eff, (W, H, nc) = _p_want(data, scale, ct, win, size, ref_fmt, flip)
        got = out[i]
        if isinstance(got, Exception):
            bad.append((i, win, repr(got)))
            continue
        if got.dtype != fmt.numpy_dtype or got.shape != want.shape or not np.array_equal(T.bits(got), want):
            bad.append((i, win, flip, (W, H, nc), got.shape, want.shape))
        assert p.window(i) == eff, (label, i, p.window(i), eff)
        assert J._native.lib().jpgpu_pipeline_pixel_bytes(p._h, i) == size[0] * size[1] * nc * fmt.itemsize, (label, i)
    assert not bad, (label, size, bad[:8], len(bad))


P_ROUTES = {
    "host-compact": ("base", {"device_entropy": False}, {}, "420"),
    "device-entry-walk": ("base", {}, {"JPGPU_PIPE_FORCE_DEVICE": "1"}, "420"),
    "device-no-entry-walk": ("base", {}, {"JPGPU_PIPE_FORCE_DEVICE": "1", "JPGPU_PIPE_ENTRY_PIXELS": "0"}, "420"),
    "device-restart-gray": ("restart", {}, {"JPGPU_PIPE_FORCE_DEVICE": "1"}, "gray"),
    "prog-device": ("prog", {}, {"JPGPU_PIPE_PROG_DEVICE_PERCENT": "100"}, "444"),
    "prog-host": ("prog", {"progressive_on_host": True}, {}, "422"),
    "host-cmyk": ("base", {"device_entropy": False}, {}, "cmyk"),
}


@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("route", sorted(P_ROUTES))
def test_pipeline_tensor_matrix(monkeypatch, route, dtype):
    enc, kwargs, env, layout = P_ROUTES[route]
    flayout, ct, sizes = PW.LAYOUTS[layout]
    files, wins = [], []
    for j, sz in enumerate(sizes):
        data = PW._file(flayout, enc, sz, pic=j)
        _full, W, H, _nc = PW._want(data, None, ct)
        for win in PW.windows_of(W, H):
            files.append(data), wins.append(win)
    flips = [(i * 7 % 3) == 0 for i in range(len(files))]
    size = (224, 224) if dtype == "float32" else (37, 53)
    fmt, ref_fmt = fmt_of(dtype)
    PW._env(monkeypatch, env)
    p = J.Pipeline(threads=4)
    try:
        out = p.decode(files, color_transform=ct, windows=wins, output_size=size, tensor=fmt, flips=flips, **kwargs)
        t = p.timings()
        _p_check(p, files, wins, flips, out, size, fmt, ref_fmt, None, ct, label=route)
        assert t["images_resized"] == t["images_ok"] == len(files), t
        assert t["pixel_bytes"] == sum(o.nbytes for o in out), t
        assert p.kernel_path.endswith("+resize+tensor") or p.kernel_path == "mixed", p.kernel_path
        if route.startswith("device"):
            assert t["images_device_entropy"] == len(files) and t["images_device_rejected"] == 0, t
            if layout == "420":
                assert (t["images_entry_pixels"] > 0) == (route == "device-entry-walk"), t
        elif route == "prog-device":
            assert t["images_device_progressive"] == len(files), t
        else:
            assert t["images_device_entropy"] == 0, t
    finally:
        p.close()


def test_pipeline_tensor_by_every_download_mode(monkeypatch):
    PW._env(monkeypatch, {})
    files = [PW._file("420", "base", (333, 200), pic=k) for k in range(6)] + [PW._file("gray", "base", (161, 97), pic=1)]
    wins = [(13, 5, 101, 77), None, (0, 0, 333, 200), (332, 199, 1, 1), (0, 7, 333, 1), (16, 16, 64, 32), (5, 3, 7, 5)]
    flips = [True, False, True, False, True, True, False]
    size = (224, 224)
    fmt, ref_fmt = fmt_of("bfloat16")
    p = J.Pipeline(threads=4)
    try:
        a = p.decode(files, windows=wins, download=True, output_size=size, tensor=fmt, flips=flips)
        _p_check(p, files, wins, flips, a, size, fmt, ref_fmt, label="download=True")
        assert p.timings()["pixel_bytes"] == sum(x.nbytes for x in a) == (6 * 3 + 1) * 224 * 224 * 2
        counts = p.decode(files, windows=wins, download="pinned", output_size=size, tensor=fmt, flips=flips)
        assert counts == [x.nbytes for x in a]
        b = [p.pixels_host(i).copy() for i in range(len(files))]
        counts = p.decode(files, windows=wins, download=False, output_size=size, tensor=fmt, flips=flips)
        assert counts == [x.nbytes for x in a] and p.pixels_host(0) is None
        c = [p.download(i) for i in range(len(files))]
        for i in range(len(files)):
            assert b[i].shape == c[i].shape == a[i].shape and np.array_equal(a[i], b[i]) and np.array_equal(a[i], c[i]), i
    finally:
        p.close()


def test_pipeline_damaged_and_planar_files_fail_alone(monkeypatch):
    PW._env(monkeypatch, {})
    good, planar = PW._file("420", "base", (333, 200)), PW._file("444", "base", (161, 97))
    gray = PW._file("gray", "base", (161, 97))
    damaged = b"\xff\xd8\xff\xe0\x00\x03"
    fmt, ref_fmt = fmt_of("float32")
    p = J.Pipeline(threads=4)
    try:
        files, flips = [good, damaged, good, gray], [True, True, False, True]
        out = p.decode(files, output_size=(32, 24), tensor=fmt, flips=flips, windows=[None, None, (300, 100, 40, 40), None])
        assert isinstance(out[1], Exception) and isinstance(out[2], J.FormatError) and "window" in str(out[2])
        for k in (0, 3):
            want, _e, _g = _p_want(files[k], None, None, None, (32, 24), ref_fmt, flips[k])
            assert np.array_equal(T.bits(out[k]), want), k
        assert p.timings()["images_ok"] == p.timings()["images_resized"] == 2
        files = [planar, gray, planar]
        out = p.decode(files, color_transform="None", output_size=(32, 24), tensor=fmt, flips=[True, True, False])
        assert isinstance(out[0], J.UnsupportedError) and "planar" in str(out[0]) and isinstance(out[2], J.UnsupportedError)
        want, _e, _g = _p_want(gray, None, "None", None, (32, 24), ref_fmt, True)
        assert np.array_equal(T.bits(out[1]), want)
        # a std of 0 for a channel only the colour image has: the gray one decodes
        odd = J.TensorFormat("float32", (0.5, 0.5, 0.5), (0.5, 0.0, 0.5))
        out = p.decode([good, gray], output_size=(32, 24), tensor=odd)
        assert isinstance(out[0], J.FormatError) and "std" in str(out[0])
        want, _e, _g = _p_want(gray, None, None, None, (32, 24), ("float32", odd.mean, odd.std), False)
        assert np.array_equal(T.bits(out[1]), want)
    finally:
        p.close()


def test_pipeline_flips_without_a_tensor_output_decode_nothing(monkeypatch):
    PW._env(monkeypatch, {})
    good = PW._file("420", "base", (333, 200))
    p = J.Pipeline(threads=4)
    try:
        for kwargs in ({}, {"output_size": (32, 24)}, {"windows": [(1, 1, 9, 9)] * 2}):
            with pytest.raises(J.FormatError, match="tensor"):
                p.decode([good, good], flips=[True, False], **kwargs)
            assert J._native.lib().jpgpu_pipeline_pixel_bytes(p._h, 0) == 0
        with pytest.raises(J.FormatError, match="output size"):
            p.decode([good, good], tensor=J.TensorFormat())
        out = p.decode([good, good])  # (and the pipeline goes on as ever)
        PW._check_call(p, [good, good], [None, None], out)
    finally:
        p.close()


def test_pipeline_fresh_windows_and_flips_keep_the_sub_batches(monkeypatch, capfd):
    """Three calls on one pipeline for the same files: fresh windows and flips each time, no sub-batch created after the first."""
    n = 64
    files = [PW._file("420", "base", (333, 200), pic=k % 8) for k in range(n)]
    fmt, ref_fmt = fmt_of("float16")
    rng = np.random.default_rng(3)
    steps = [("A", True), ("B", True), ("B", True), ("C", False), ("C", True)]
    p = J.Pipeline(threads=4)
    try:
        for c, (wname, flipped) in enumerate(steps):
            PW._env(monkeypatch, {})
            monkeypatch.setenv("JPGPU_PIPE_TRACE", "1")
            wins = PW._windows_set(wname, n)
            flips = [bool(v) for v in rng.integers(0, 2, n)] if flipped else None
            capfd.readouterr()
            out = p.decode(files, windows=wins, output_size=(64, 48), tensor=fmt, flips=flips)
            trace = capfd.readouterr().err
            _p_check(p, files, wins, flips, out, (64, 48), fmt, ref_fmt, label=f"call {c}")
            assert "sub-batch" in trace
            if c:
                assert "created" not in trace and ("kept" in trace or "re-windowed" in trace), (c, trace[-600:])
                assert ("re-windowed in place" in trace) == (steps[c - 1][0] != wname), (c, trace[-600:])
    finally:
        monkeypatch.delenv("JPGPU_PIPE_TRACE", raising=False)
        p.close()


def test_pipeline_tensor_on_off_and_other_dtype_between_calls(monkeypatch, capfd):
    n = 16
    size = (48, 32)
    wins = PW._windows_set("A", n)
    steps = ["float32", None, "float16", "float16", "bfloat16", None, "float32"]
    p = J.Pipeline(threads=4)
    try:
        for c, dtype in enumerate(steps):
            PW._env(monkeypatch, {})
            monkeypatch.setenv("JPGPU_PIPE_TRACE", "1")
            files = [PW._file("420", "base", (333, 200), pic=(k + 4 * (c % 2)) % 8) for k in range(n)]
            flips = None if dtype is None else [(k + c) % 2 == 0 for k in range(n)]
            capfd.readouterr()
            if dtype is None:
                out = p.decode(files, windows=wins, output_size=size)
                RZ._p_check(p, files, wins, out, size, label=f"call {c}")
                assert p.kernel_path.endswith("+resize")
            else:
                fmt, ref_fmt = fmt_of(dtype)
                out = p.decode(files, windows=wins, output_size=size, tensor=fmt, flips=flips)
                _p_check(p, files, wins, flips, out, size, fmt, ref_fmt, label=f"call {c}")
                assert p.kernel_path.endswith("+resize+tensor")
            trace = capfd.readouterr().err
            if c:
                assert ("created" in trace) == (steps[c - 1] != dtype), (c, trace[-600:])
    finally:
        monkeypatch.delenv("JPGPU_PIPE_TRACE", raising=False)
        p.close()


@pytest.mark.parametrize("gather", [False, True], ids=["plain", "gather"])
def test_pipeline_tensor_two_children_on_one_device(monkeypatch, gather):
    PW._env(monkeypatch, {})
    n = 48
    size = (37, 53)
    files = [PW._file("420", "base", (333, 200) if k % 3 else (161, 97), pic=k % 8) for k in range(n)]
    wins = [None if k % 5 == 0 else ((13 + k, 5 + k % 9, 41 + 2 * (k % 20), 33) if k % 3 else (5, 3, 7 + 2 * (k % 30), 5 + k % 40)) for k in range(n)]
    flips = [k % 3 != 1 for k in range(n)]  # (image i goes to child i mod 2: both children get both kinds)
    fmt, ref_fmt = fmt_of("float32")
    p = J.Pipeline(devices=[0, 0], threads=4)
    try:
        p.decode(files, windows=wins, gather=gather, download=False, output_size=size, tensor=fmt, flips=flips)
        t = p.timings()
        assert t["images_ok"] == t["images_resized"] == n and t["pixel_bytes"] == n * 37 * 53 * 3 * 4, t
        got = [p.download(i) for i in range(n)]
        _p_check(p, files, wins, flips, got, size, fmt, ref_fmt, label="two children")
        if gather:
            assert t["gather_bytes"] > 0, t
            hip = _hip()
            for i in range(n):
                buf = np.empty(got[i].nbytes, np.uint8)
                assert hip.hipMemcpy(buf.ctypes.data, p.device_pointer(i), buf.size, 2) == 0
                assert np.array_equal(buf.view(np.uint32), T.bits(got[i]).reshape(-1)), i
        out = p.decode(files, windows=wins, gather=gather, output_size=size, tensor=fmt, flips=flips)
        _p_check(p, files, wins, flips, out, size, fmt, ref_fmt, label="two children, downloaded")
    finally:
        p.close()


def test_pipeline_256_files_of_1080p_random_resized_crops_and_flips_to_224_f16(monkeypatch):
    """A loader's call: 256 files, a RandomResizedCrop window and a random flip each, 3 x 224 x 224 f16 per image in the pinned block —
    every image compared."""
    PW._env(monkeypatch, {})
    n, distinct = 256, 4
    pics = [PW.BE.synthetic_jpeg(1920, 1080, seed=9000 + k) for k in range(distinct)]
    fulls = [O.decode(d).pixels.reshape(1080, 1920, 3) for d in pics]
    rng = np.random.default_rng(20261017)
    wins = PW.random_resized_crops(rng, n, 1920, 1080)
    flips = [bool(v) for v in rng.integers(0, 2, n)]
    files = [pics[k % distinct] for k in range(n)]
    fmt, ref_fmt = fmt_of("float16", T.IMAGENET)
    tab = T.table(ref_fmt, 3)
    p = J.Pipeline()
    try:
        counts = p.decode(files, windows=wins, download="pinned", output_size=(224, 224), tensor=fmt, flips=flips)
        t = p.timings()
        assert t["images_ok"] == t["images_resized"] == n and t["images_device_rejected"] == 0, t
        assert t["pixel_bytes"] == n * 3 * 224 * 224 * 2 and counts == [3 * 224 * 224 * 2] * n
        bad = []
        for i, (x, y, w, h) in enumerate(wins):
            want = T.to_tensor(R.resize(fulls[i % distinct][y:y + h, x:x + w], 224, 224), tab, flips[i])
            got = p.pixels_host(i)
            if got.shape != (3, 224, 224) or hashlib.sha256(T.bits(want)).digest() != hashlib.sha256(T.bits(got)).digest():
                bad.append((i, wins[i], flips[i]))
        assert not bad, (bad[:10], len(bad))
    finally:
        p.close()
