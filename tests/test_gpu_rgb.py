"""RGB output on the GPU: Batch(output_size=, rgb=True) and Pipeline.decode(output_size=, rgb=True) against
tests/resample_ref.py of tests/rgb_ref.py of the oracle's decode — convert, then crop, then resample — bit for bit, as bytes and as
tensors.  The helpers are those of tests/test_gpu_resize.py and tests/test_gpu_tensor.py."""
import ctypes as C

import numpy as np
import pytest

import resample_ref as R
import rgb_ref as G
import tensor_ref as T
import test_gpu_pipeline_windows as PW
import test_gpu_resize as RZ
import test_gpu_tensor as TN
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
    TN.J = pkg
    assert J.device_count() >= 1, "no MI355X visible: the HIP path has no CPU fallback"


def want_u8(case, full, win, size):
    return R.resize(G.to_rgb(RZ.source_of(case, full, win)), size[0], size[1])


def want_tensor(u8, ref_fmt, flip):
    return T.bits(T.to_tensor(u8, T.table(ref_fmt, 3), flip))


def _decode(cases, wins, size, fmt=None, flips=None, rgb=True):
    b = J.Batch([RZ._desc(c) for c in cases], windows=wins, output_size=size, tensor=fmt, rgb=rgb)
    try:
        RZ._upload(b, cases)
        if flips is not None:
            b.set_flips(flips)
        b.decode()
        b.synchronize()
        es = 1 if fmt is None else fmt.itemsize
        for i in range(len(cases)):
            assert b.out_bytes(i) == size[0] * size[1] * 3 * es and b.out_offset(i) % 256 == 0
        return [b.download(i) for i in range(len(cases))], b.path
    finally:
        b.close()


# Grayscale, CMYK 4:4:4, YCCK with half-size chroma, YCbCr 4:2:0, RGB
LAYOUTS = [([(1, 1)], "Grayscale"), ([(1, 1)] * 4, "CMYK"), ([(2, 2), (1, 1), (1, 1), (2, 2)], "YCCK"), ([(2, 2), (1, 1), (1, 1)], "YCbCr"), ([(1, 1)] * 3, "RGB")]
SIZES = [(1, 1), (17, 9), (161, 97), (50, 34), (640, 480)]
OUT_SIZES = [(224, 224), (1, 1), (37, 53), (2048, 3)]
_MIXED = {}


def _mixed():
    """One call of every layout at every size with the windows of RZ._windows, and the u8 references: made once, never changed."""
    if not _MIXED:
        rng = np.random.default_rng(1200)
        cases, wins, fulls = [], [], []
        for k, (samp, ct) in enumerate(LAYOUTS):
            for n, (w_, h_) in enumerate(SIZES):
                case = RZ._case(rng, w_, h_, samp, ct, 8, "hostile" if n == 2 and k == 1 else "sparse")
                full = RZ._full(case)
                oc, *_r, ow, oh = case
                W, H = grid_of(oc, ow, oh)
                win = RZ._windows(W, H, n + k)[(n + k) % 2]
                cases.append(case), wins.append(win), fulls.append(full)
        _MIXED["call"] = (cases, wins, fulls)
        _MIXED["u8"] = {size: [want_u8(c, f, w, size) for c, w, f in zip(cases, wins, fulls)] for size in OUT_SIZES}
    return _MIXED["call"], _MIXED["u8"]


@pytest.mark.parametrize("dtype", [None, "float32", "float16", "bfloat16"], ids=lambda d: d or "u8")
def test_mixed_channel_launch_bit_exact(dtype):
    (cases, wins, fulls), u8 = _mixed()
    assert {len(c[0]) for c in cases} == {1, 3, 4} and len(cases) == 25
    flips = [i % 2 == 1 for i in range(len(cases))]
    for size in OUT_SIZES:
        if dtype is None:
            outs, path = _decode(cases, wins, size)
            assert path == "mixed+rgb+resize", path
            for i, o in enumerate(outs):
                assert o.dtype == np.uint8 and o.shape == (size[0] * size[1] * 3,)
                assert np.array_equal(o, u8[size][i].reshape(-1)), (i, cases[i][3], wins[i], size, np.nonzero(o != u8[size][i].reshape(-1))[0][:8].tolist())
        else:
            fmt, ref_fmt = TN.fmt_of(dtype)
            outs, path = _decode(cases, wins, size, fmt, flips)
            assert path == "mixed+rgb+resize+tensor", path
            for i, o in enumerate(outs):
                want = want_tensor(u8[size][i], ref_fmt, flips[i])
                assert o.dtype == fmt.numpy_dtype and o.shape == (3, size[1], size[0]), (i, o.shape)
                assert np.array_equal(T.bits(o), want), (i, cases[i][3], wins[i], size, flips[i], np.argwhere(T.bits(o) != want)[:6].tolist())


def test_chunked_vertical_path():
    rng = np.random.default_rng(12)
    cases = [RZ._case(rng, 24, 2000, [(1, 1)], "Grayscale"), RZ._case(rng, 16, 1200, [(1, 1)] * 4, "CMYK")] * 2
    fulls = [RZ._full(c) for c in cases[:2]] * 2
    flips = [False, False, True, True]
    for size in [(2048, 1), (333, 1)]:
        u8 = [want_u8(c, f, None, size) for c, f in zip(cases[:2], fulls)] * 2
        outs, _p = _decode(cases, None, size)
        for i in range(4):
            assert np.array_equal(outs[i], u8[i].reshape(-1)), (size, i)
        for dtype in ("float32", "bfloat16"):
            fmt, ref_fmt = TN.fmt_of(dtype)
            outs, _p = _decode(cases, None, size, fmt, flips)
            for i in range(4):
                assert np.array_equal(T.bits(outs[i]), want_tensor(u8[i], ref_fmt, flips[i])), (size, dtype, i)


def test_callers_arena_is_one_contiguous_n_3_224_224_tensor():
    """A caller's EXTERNAL_BUFFERS arena poisoned with two patterns: gray, CMYK and colour images to (224, 224) f32 follow each other
    without a gap, every element is written, no byte beyond the arena changes."""
    hip = TN._hip()
    rng = np.random.default_rng(77)
    layouts = [([(1, 1)], "Grayscale"), ([(2, 2), (1, 1), (1, 1)], "YCbCr"), ([(1, 1)] * 4, "CMYK"), ([(1, 1)] * 3, "RGB"), ([(2, 2), (1, 1), (1, 1), (2, 2)], "YCCK"),
               ([(1, 1)], "Grayscale")]
    sizes = [(250, 130), (333, 200), (64, 48), (33, 17), (161, 97), (9, 300)]
    cases = [RZ._case(rng, w_, h_, samp, ct) for (samp, ct), (w_, h_) in zip(layouts, sizes)]
    wins = [None, (101, 53, 133, 117), (1, 1, 61, 45), (3, 1, 29, 15), None, (2, 7, 5, 201)]
    flips = [True, False, True, True, False, True]
    fulls = [RZ._full(c) for c in cases]
    size, n = (224, 224), len(cases)
    fmt, ref_fmt = TN.fmt_of("float32")
    wants = [want_tensor(want_u8(c, f, w, size), ref_fmt, fl) for c, f, w, fl in zip(cases, fulls, wins, flips)]
    b = J.Batch([RZ._desc(c) for c in cases], flags=J._native.BATCH_EXTERNAL_BUFFERS, windows=wins, output_size=size, tensor=fmt, rgb=True)
    coef, out = C.c_void_p(), C.c_void_p()
    nco, nout = b.coef_arena_bytes(), b.out_arena_bytes()
    assert nout == n * 3 * 224 * 224 * 4
    assert [b.out_offset(i) for i in range(n)] == [i * 3 * 224 * 224 * 4 for i in range(n)]
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
            got = host[:nout].view(np.uint32).reshape(n, 3, 224, 224)
            for i in range(n):
                assert np.array_equal(got[i], wants[i]), (hex(pattern), i, wins[i])
            assert (host[nout:] == pattern).all(), "the kernel wrote behind the arena"
    finally:
        b.close()
        hip.hipFree(coef)
        hip.hipFree(out)


def test_set_flips_and_new_coefficients_on_a_reused_batch():
    rng = np.random.default_rng(8)
    layouts = [([(1, 1)], "Grayscale"), ([(1, 1)] * 4, "CMYK"), ([(2, 2), (1, 1), (1, 1)], "YCbCr")]
    sizes = [(50, 34), (161, 97), (64, 64)]
    first = [RZ._case(rng, w_, h_, samp, ct) for (samp, ct), (w_, h_) in zip(layouts, sizes)]
    second = [RZ._case(rng, w_, h_, samp, ct) for (samp, ct), (w_, h_) in zip(layouts, sizes)]
    wins = [None, (3, 5, 101, 77), (1, 1, 9, 60)]
    size = (40, 24)
    fmt, ref_fmt = TN.fmt_of("float16")
    b = J.Batch([RZ._desc(c) for c in first], windows=wins, output_size=size, tensor=fmt, rgb=True)
    try:
        offs = [b.out_offset(i) for i in range(3)]
        for cases, flips in ((first, None), (first, [True, False, True]), (second, [False, True, True]), (second, None)):
            for i, (oc, qts, *_r) in enumerate(cases):
                for c in range(len(oc)):
                    b.set_quantization_table(i, c, qts[c])
            RZ._upload(b, cases)
            b.set_flips(flips)
            b.decode()
            b.synchronize()
            for i, case in enumerate(cases):
                want = want_tensor(want_u8(case, RZ._full(case), wins[i], size), ref_fmt, bool(flips[i]) if flips else False)
                assert np.array_equal(T.bits(b.download(i)), want), (i, flips)
            assert offs == [b.out_offset(i) for i in range(3)]
    finally:
        b.close()


def test_refusals():
    rng = np.random.default_rng(1)
    gray = RZ._case(rng, 64, 48, [(1, 1)], "Grayscale")
    colour = RZ._case(rng, 64, 48, [(2, 2), (1, 1), (1, 1)], "YCbCr")
    planar = RZ._case(rng, 64, 48, [(1, 1)] * 3, "None")
    with pytest.raises(J.UnsupportedError, match="output size"):
        J.Batch([RZ._desc(gray)], rgb=True)
    with pytest.raises(J.UnsupportedError, match="output size"):
        J.Batch([RZ._desc(gray)], windows=[(1, 1, 9, 9)], rgb=True)
    with pytest.raises(J.UnsupportedError, match="planar"):
        J.Batch([RZ._desc(colour), RZ._desc(planar)], output_size=(8, 8), rgb=True)
    odd = J.TensorFormat("float16", (0.5,) * 3, (0.5, 0.5, 0.0))
    with pytest.raises(J.FormatError, match="std"):  # (a gray image has three planes now)
        J.Batch([RZ._desc(gray)], output_size=(8, 8), tensor=odd, rgb=True)
    J.Batch([RZ._desc(gray)], output_size=(8, 8), tensor=odd).close()  # (and one without the option, as before)
    # the fourth channel is nobody's business, a CMYK image in the call or not
    cmyk = RZ._case(rng, 64, 48, [(1, 1)] * 4, "CMYK")
    J.Batch([RZ._desc(cmyk)], output_size=(8, 8), tensor=J.TensorFormat("float16", (0.5,) * 4, (0.5, 0.5, 0.5, 0.0)), rgb=True).close()


def test_unchanged_without_the_option():
    """The cases of test_gpu_tensor.py::test_batch_without_a_tensor_is_what_it_was: same path, same bytes."""
    rng = np.random.default_rng(21)
    cases = [RZ._case(rng, 640, 480, [(2, 2), (1, 1), (1, 1)], "YCbCr"), RZ._case(rng, 300, 200, [(1, 1)], "Grayscale")]
    wins = [(100, 50, 333, 217), None]
    fulls = [RZ._full(c) for c in cases]
    outs, path = RZ._decode(cases, wins, (224, 224))
    assert path == "mixed+resize"
    RZ._check(outs, cases, wins, fulls, (224, 224))
    b = J.Batch([RZ._desc(c) for c in cases], output_size=(224, 224))
    assert b.rgb is False and b.out_bytes(1) == 224 * 224 and b.out_arena_bytes() == 224 * 224 * 3 + 224 * 224
    b.close()
    outs, path = _decode(cases, wins, (224, 224))
    assert path == "mixed+rgb+resize" and outs[1].size == 224 * 224 * 3
    assert np.array_equal(outs[0], RZ.want_resized(cases[0], fulls[0], wins[0], (224, 224)))  # (three channels: what they were)


# ======================================================== Pipeline ========================================================================
P_ROUTES = {
    "host-compact": ({"device_entropy": False}, {}, "base"),
    "device-entry-walk": ({}, {"JPGPU_PIPE_FORCE_DEVICE": "1"}, "base"),
    "device-no-entry-walk": ({}, {"JPGPU_PIPE_FORCE_DEVICE": "1", "JPGPU_PIPE_ENTRY_PIXELS": "0"}, "base"),
    "device-restart-gray": ({}, {"JPGPU_PIPE_FORCE_DEVICE": "1"}, "restart"),
}
_P_FILES = {}


def _p_files(gray_enc):
    """Gray, CMYK, YCCK, YCCK with half-size chroma and 4:2:0 files for ONE call, each with the windows of PW.windows_of."""
    if gray_enc not in _P_FILES:
        files, wins = [], []
        for layout in ("gray", "cmyk", "ycck", "ycck-half", "420"):
            flayout, _ct, sizes = PW.LAYOUTS[layout]
            enc = gray_enc if layout == "gray" else ("prog" if layout == "ycck-half" else "base")
            for j, sz in enumerate(sizes):
                data = PW._file(flayout, enc, sz, pic=j)
                _full, W, H, _nc = PW._want(data, None, None)
                for win in PW.windows_of(W, H)[j::2]:
                    files.append(data), wins.append(win)
        _P_FILES[gray_enc] = (files, wins)
    return _P_FILES[gray_enc]


def _p_u8(data, win, size):
    src, eff, geom = RZ._p_source(data, None, None, win)
    return R.resize(G.to_rgb(src), size[0], size[1]), eff, geom


def _p_check(p, files, wins, flips, out, size, fmt, ref_fmt, label=""):
    bad, ncs = [], set()
    es = 1 if fmt is None else fmt.itemsize
    for i, data in enumerate(files):
        win = None if wins is None else wins[i]
        u8, eff, (W, H, nc) = _p_u8(data, win, size)
        ncs.add(nc)
        got = out[i]
        if isinstance(got, Exception):
            bad.append((i, win, repr(got)))
            continue
        if fmt is None:
            ok = got.dtype == np.uint8 and got.shape == (size[0] * size[1] * 3,) and np.array_equal(got, u8.reshape(-1))
        else:
            want = want_tensor(u8, ref_fmt, bool(flips[i]) if flips is not None else False)
            ok = got.dtype == fmt.numpy_dtype and got.shape == (3, size[1], size[0]) and np.array_equal(T.bits(got), want)
        if not ok:
            bad.append((i, win, (W, H, nc), got.shape))
        assert p.window(i) == eff, (label, i, p.window(i), eff)
        assert J._native.lib().jpgpu_pipeline_pixel_bytes(p._h, i) == size[0] * size[1] * 3 * es, (label, i)
        assert p.info(i).pixel_format == {1: "L8", 3: "RGB24", 4: "CMYK32"}[nc], (label, i, p.info(i))  # (the file's own)
    assert not bad, (label, size, bad[:8], len(bad))
    return ncs


@pytest.mark.parametrize("dtype", [None, "float32", "float16"], ids=lambda d: d or "u8")
@pytest.mark.parametrize("route", sorted(P_ROUTES))
def test_pipeline_rgb_matrix(monkeypatch, route, dtype):
    kwargs, env, gray_enc = P_ROUTES[route]
    files, wins = _p_files(gray_enc)
    flips = None if dtype is None else [(i * 7 % 3) == 0 for i in range(len(files))]
    size = (37, 53) if dtype == "float16" else (224, 224)
    fmt, ref_fmt = (None, None) if dtype is None else TN.fmt_of(dtype)
    PW._env(monkeypatch, env)
    p = J.Pipeline(threads=4)
    try:
        out = p.decode(files, windows=wins, output_size=size, tensor=fmt, flips=flips, rgb=True, **kwargs)
        t = p.timings()
        assert _p_check(p, files, wins, flips, out, size, fmt, ref_fmt, label=route) == {1, 3, 4}
        assert t["images_resized"] == t["images_ok"] == len(files), t
        assert t["pixel_bytes"] == sum(o.nbytes for o in out) == len(files) * size[0] * size[1] * 3 * (1 if fmt is None else fmt.itemsize), t
        assert "+rgb+resize" in p.kernel_path or p.kernel_path == "mixed", p.kernel_path
        if route.startswith("device"):
            assert t["images_device_entropy"] > 0, t
            if route == "device-no-entry-walk":
                assert t["images_entry_pixels"] == 0, t
        else:
            assert t["images_device_entropy"] == 0, t
    finally:
        p.close()


def test_pipeline_rgb_by_every_download_mode(monkeypatch):
    PW._env(monkeypatch, {})
    files, wins = _p_files("base")
    files, wins = files[::3], wins[::3]
    flips = [i % 2 == 0 for i in range(len(files))]
    size = (64, 48)
    fmt, ref_fmt = TN.fmt_of("bfloat16")
    p = J.Pipeline(threads=4)
    try:
        a = p.decode(files, windows=wins, download=True, output_size=size, tensor=fmt, flips=flips, rgb=True)
        assert _p_check(p, files, wins, flips, a, size, fmt, ref_fmt, label="download=True") == {1, 3, 4}
        assert p.timings()["pixel_bytes"] == len(files) * 3 * 64 * 48 * 2
        counts = p.decode(files, windows=wins, download="pinned", output_size=size, tensor=fmt, flips=flips, rgb=True)
        assert counts == [x.nbytes for x in a]
        b = [p.pixels_host(i).copy() for i in range(len(files))]
        counts = p.decode(files, windows=wins, download=False, output_size=size, tensor=fmt, flips=flips, rgb=True)
        assert counts == [x.nbytes for x in a] and p.pixels_host(0) is None
        c = [p.download(i) for i in range(len(files))]
        for i in range(len(files)):
            assert b[i].shape == c[i].shape == a[i].shape == (3, 48, 64) and np.array_equal(a[i], b[i]) and np.array_equal(a[i], c[i]), i
    finally:
        p.close()


def test_pipeline_option_off_and_on_again_and_fresh_windows_in_place(monkeypatch, capfd):
    """One Pipeline, the same files: the option toggled creates the sub-batches anew (like another output size) and every call is exact;
    fresh windows and flips with the option on are set in place."""
    files, wins = _p_files("base")
    files, wins = files[::2], wins[::2]
    n = len(files)
    # (other windows for the SAME set of windowed images: one that starts at the origin may be the whole image — left as it is)
    other = [w if (w is None or (w[0] == 0 and w[1] == 0)) else (w[0], w[1], max(1, w[2] - 1), max(1, w[3] - 1)) for w in wins]
    size = (48, 32)
    fmt, ref_fmt = TN.fmt_of("float32")
    steps = [(True, wins), (False, wins), (True, wins), (True, other), (False, other)]
    p = J.Pipeline(threads=4)
    try:
        for c, (rgb, ws) in enumerate(steps):
            PW._env(monkeypatch, {})
            monkeypatch.setenv("JPGPU_PIPE_TRACE", "1")
            flips = [(k + c) % 2 == 0 for k in range(n)]
            capfd.readouterr()
            out = p.decode(files, windows=ws, output_size=size, tensor=fmt, flips=flips, rgb=rgb)
            trace = capfd.readouterr().err
            if rgb:
                _p_check(p, files, ws, flips, out, size, fmt, ref_fmt, label=f"call {c}")
            else:
                TN._p_check(p, files, ws, flips, out, size, fmt, ref_fmt, label=f"call {c}")
                assert {o.shape[0] for o in out} == {1, 3, 4}
            if c:
                assert ("created" in trace) == (steps[c - 1][0] != rgb), (c, trace[-600:])
            if c == 3:
                assert "re-windowed in place" in trace, trace[-600:]
    finally:
        monkeypatch.delenv("JPGPU_PIPE_TRACE", raising=False)
        p.close()


def test_pipeline_rgb_without_an_output_size_decodes_nothing(monkeypatch):
    PW._env(monkeypatch, {})
    good = PW._file("gray", "base", (161, 97))
    p = J.Pipeline(threads=4)
    try:
        for kwargs in ({}, {"windows": [(1, 1, 9, 9)] * 2}):
            with pytest.raises(J.FormatError, match="output size"):
                p.decode([good, good], rgb=True, **kwargs)
            assert J._native.lib().jpgpu_pipeline_pixel_bytes(p._h, 0) == 0
        out = p.decode([good, good])  # (and the pipeline goes on as ever)
        PW._check_call(p, [good, good], [None, None], out)
        out = p.decode([good, good], output_size=(8, 8), rgb=True)
        assert all(o.size == 8 * 8 * 3 for o in out)
    finally:
        p.close()
