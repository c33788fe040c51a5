"""Colour operations from JPEG bytes (jpgpu_pipeline_set_colour, jpgpu_pipeline_decode_coloured) on the MI355X: fresh programs on every
call of a loader, set in place in the kept sub-batches of one Pipeline.  The expected value is tests/colour_ref.py
applied to the reference result the resize, warp and tensor tests of the pipeline use, compared with np.array_equal."""
import ctypes as C

import numpy as np
import pytest

import colour_ref as CR
import filter_ref as F
import rgb_ref as G
import tensor_ref as T
import test_gpu_pipeline_windows as PW
import test_gpu_resize as RZ
import test_gpu_tensor as TN
import warp_ref as WR

pytestmark = pytest.mark.gpu

J = None
SIZE = (33, 21)
WFILL = (9, 250, 77, 140)
GEOM = (97, 61)
OPS = [("brightness", (0.0, 0.37, 1.0, 1.9)), ("contrast", (0.0, 0.37, 1.9)), ("saturation", (0.0, 0.37, 1.9)), ("solarize", (0, 100, 128, 256)),
       ("posterize", (1, 3, 8)), ("invert", (0,)), ("autocontrast", (0,)), ("equalize", (0,)), ("identity", (0,))]


@pytest.fixture(scope="module", autouse=True)
def _load():
    global J
    import jpeg_decoder_amd as pkg
    J = pkg
    PW.J = pkg
    RZ.J = pkg
    TN.J = pkg
    assert J.device_count() >= 1, "no MI355X visible: the HIP path has no CPU fallback"


def files():
    """Twelve small three-component files: 4:2:0 and 4:4:4, baseline and progressive, and two reftest files."""
    kinds = [("420", "base"), ("420", "prog"), ("444", "base"), ("444", "prog")]
    return [PW._file(*kinds[k % 4], GEOM, pic=k) for k in range(10)] + [PW._golden("reftest", "mozilla", "jpg-size-33x33.jpg"), PW._golden("reftest", "restarts.jpg")]


def fresh(rng, n):
    """The programs of one call: 0..4 operations per image."""
    out = []
    for _ in range(n):
        prog = []
        for _k in range(int(rng.integers(0, 5))):
            name, values = OPS[int(rng.integers(0, len(OPS)))]
            prog.append((name, float(values[int(rng.integers(0, len(values)))])))
        out.append(prog if prog or rng.integers(0, 2) else None)
    return out


def resized(data, win=None, rgb=False):
    src, _eff, _g = RZ._p_source(data, None, None, win)
    return F.resize(G.to_rgb(src) if rgb else src, SIZE[0], SIZE[1], F.BILINEAR)


def want_u8(data, program, win=None, flip=False, m=None, filt=None, rgb=False):
    r = resized(data, win, rgb)
    c = CR.apply(r, program) if r.shape[2] == 3 else r
    c = c[:, ::-1] if flip else c
    if filt is None:
        return np.ascontiguousarray(c)
    return WR.warp(c, WR.IDENTITY if m is None else m, WR.BILINEAR if filt == "bilinear" else WR.NEAREST, WFILL)


def test_fresh_programs_keep_the_sub_batches(monkeypatch, capfd):
    """Programs, flips and matrices change on every call; the trace shows the sub-batches kept."""
    fs = files()
    fmt, ref_fmt = TN.fmt_of("float32")
    rng = np.random.default_rng(20)
    p = J.Pipeline(threads=4)
    try:
        for c in range(4):
            PW._env(monkeypatch, {})
            monkeypatch.setenv("JPGPU_PIPE_TRACE", "1")
            programs = fresh(rng, len(fs))
            flips = [bool(v) for v in rng.integers(0, 2, len(fs))]
            warps = [None if k % 3 == 0 else WR.rotate_matrix(float(rng.uniform(-40, 40)), SIZE) for k in range(len(fs))]
            capfd.readouterr()
            out = p.decode(fs, output_size=SIZE, tensor=fmt, flips=flips, warp=J.WarpOptions("bilinear", WFILL), warps=warps, colour=True, colours=programs)
            trace = capfd.readouterr().err
            assert "sub-batch" in trace and "+colour+warp:bilinear+tensor" in p.kernel_path, p.kernel_path
            if c:
                assert "created" not in trace and "kept" in trace, (c, trace[-600:])
            for i, data in enumerate(fs):
                assert not isinstance(out[i], Exception), (c, i, out[i])
                u8 = want_u8(data, programs[i], None, flips[i], warps[i], "bilinear")
                assert np.array_equal(T.bits(out[i]), T.bits(T.to_tensor(u8, T.table(ref_fmt, 3), False))), (c, i, programs[i], flips[i], warps[i])
    finally:
        monkeypatch.delenv("JPGPU_PIPE_TRACE", raising=False)
        p.close()


def test_u8_output_without_a_warp_and_colour_switched_off(monkeypatch, capfd):
    fs = files()[:8]
    rng = np.random.default_rng(21)
    p = J.Pipeline(threads=4)
    try:
        PW._env(monkeypatch, {})
        monkeypatch.setenv("JPGPU_PIPE_TRACE", "1")
        for c in range(2):
            programs = fresh(rng, len(fs))
            capfd.readouterr()
            out = p.decode(fs, output_size=SIZE, colour=True, colours=programs)
            trace = capfd.readouterr().err
            assert p.kernel_path.endswith("+resize+colour") and ("created" not in trace) == bool(c), (c, p.kernel_path)
            for i, data in enumerate(fs):
                assert np.array_equal(out[i], want_u8(data, programs[i]).reshape(-1)), (c, i, programs[i])
        plain = [resized(d).reshape(-1) for d in fs]
        capfd.readouterr()
        out = p.decode(fs, output_size=SIZE, colour=True)  # (no programs: empty ones, set in place)
        assert "created" not in capfd.readouterr().err
        for i in range(len(fs)):
            assert np.array_equal(out[i], plain[i]), i
        out = p.decode(fs, output_size=SIZE)  # (off: the sub-batches of the output size alone, created anew)
        assert "created" in capfd.readouterr().err and "colour" not in p.kernel_path
        for i in range(len(fs)):
            assert np.array_equal(out[i], plain[i]), i
    finally:
        monkeypatch.delenv("JPGPU_PIPE_TRACE", raising=False)
        p.close()


def test_no_programs_argument_is_decode_warped(monkeypatch):
    """colours=None without colour: the call, the path and the bytes of jpgpu_pipeline_decode_warped."""
    PW._env(monkeypatch, {})
    fs = files()[:6]
    warps = [WR.rotate_matrix(10.0 * k, SIZE) for k in range(len(fs))]
    p, q = J.Pipeline(threads=4), J.Pipeline(threads=4)
    try:
        a = p.decode(fs, output_size=SIZE, warp=J.WarpOptions("nearest", WFILL), warps=warps)
        path_a = p.kernel_path
        L = J._native.lib()
        n = len(fs)
        ptrs = (C.c_char_p * n)(*fs)
        lens = (C.c_size_t * n)(*[len(f) for f in fs])
        wo = J.WarpOptions("nearest", WFILL).struct()
        assert L.jpgpu_pipeline_set_output_size(q._h, *SIZE) == 0 and L.jpgpu_pipeline_set_warp(q._h, C.byref(wo)) == 0
        st = L.jpgpu_pipeline_decode_coloured(q._h, C.cast(ptrs, C.POINTER(C.c_void_p)), lens, None, None, J.batch.warp_structs(warps, n), None, n,
                                              J._native.PIPELINE_DOWNLOAD | J._native.PIPELINE_DEVICE_ENTROPY)
        assert st == 0 and L.jpgpu_pipeline_kernel_path(q._h).decode() == path_a and "colour" not in path_a
        for i in range(n):
            nbytes = L.jpgpu_pipeline_pixel_bytes(q._h, i)
            got = np.ctypeslib.as_array(C.cast(L.jpgpu_pipeline_pixels_host(q._h, i), C.POINTER(C.c_uint8)), shape=(nbytes,))
            assert np.array_equal(got, a[i]) and np.array_equal(a[i], want_u8(fs[i], None, None, False, warps[i], "nearest").reshape(-1)), i
    finally:
        p.close()
        q.close()


def test_a_refused_program_and_a_gray_file_fail_alone(monkeypatch):
    PW._env(monkeypatch, {})
    gray, cmyk = PW._file("gray", "base", GEOM, pic=3), PW._golden("reftest", "mozilla", "jpg-cmyk-1.jpg")
    fs = files()[:5] + [gray, gray, cmyk]
    good = [("contrast", 1.9), ("equalize", 0)]
    programs = [good, [("solarize", 1.5)], None, [("invert", 0)] * 5, good, good, None, [("invert", 0)]]
    p = J.Pipeline(threads=4)
    try:
        out = p.decode(fs, output_size=SIZE, colour=True, colours=programs)
        for i in (1, 3):
            assert isinstance(out[i], J.FormatError) and "colour" in str(out[i]), (i, out[i])
        for i in (5, 7):
            assert isinstance(out[i], J.UnsupportedError) and "three output channels" in str(out[i]), (i, out[i])
        for i in (0, 2, 4, 6):
            assert np.array_equal(out[i], want_u8(fs[i], programs[i]).reshape(-1)), i
        assert p.timings()["images_ok"] == 4
        # under RGB output the gray and the CMYK file take their programs
        programs = [good, None, None, [("saturation", 0.37)], good, good, [("autocontrast", 0)], [("invert", 0), ("equalize", 0)]]
        out = p.decode(fs, output_size=SIZE, rgb=True, colour=True, colours=programs)
        for i, data in enumerate(fs):
            assert np.array_equal(out[i], want_u8(data, programs[i], rgb=True).reshape(-1)), i
    finally:
        p.close()


def test_programs_without_colour_and_colour_without_an_output_size_decode_nothing(monkeypatch):
    PW._env(monkeypatch, {})
    fs = files()[:2]
    p = J.Pipeline(threads=4)
    try:
        for kwargs in ({}, {"output_size": SIZE}):
            with pytest.raises(J.FormatError, match="colour options"):
                p.decode(fs, colours=[None, [("invert", 0)]], **kwargs)
            assert J._native.lib().jpgpu_pipeline_pixel_bytes(p._h, 0) == 0
        with pytest.raises(J.FormatError, match="output size"):
            p.decode(fs, colour=True)
        with pytest.raises(ValueError):
            p.decode(fs, output_size=SIZE, colour=True, colours=[None])
        bad = J._native.ColourOptionsStruct(1)
        assert J._native.lib().jpgpu_pipeline_set_colour(p._h, C.byref(bad)) == J._native.ERR_FORMAT
        out = p.decode(fs)  # (and the pipeline goes on as ever)
        PW._check_call(p, fs, [None, None], out)
    finally:
        p.close()
