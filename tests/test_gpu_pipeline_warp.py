"""Affine warps from JPEG bytes (jpgpu_pipeline_set_warp, jpgpu_pipeline_decode_warped) on the MI355X: fresh windows, flips and matrices
on every call of a loader, set in place in the kept sub-batches.  The expected value is tests/warp_ref.py applied to
the reference result the resize and tensor tests of the pipeline use, compared with np.array_equal."""
import ctypes as C

import numpy as np
import pytest

import filter_ref as F
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
    """Twelve small files: 4:2:0 and gray, baseline and progressive."""
    kinds = [("420", "base"), ("420", "prog"), ("gray", "base"), ("gray", "prog")]
    return [PW._file(*kinds[k % 4], GEOM, pic=k) for k in range(12)]


def fresh(rng, n):
    """Windows (every image windowed: the set of windowed images repeats), flips and matrices of one call."""
    wins = [(int(rng.integers(0, 30)), int(rng.integers(0, 20)), int(rng.integers(20, 60)), int(rng.integers(15, 40))) for _ in range(n)]
    flips = [bool(v) for v in rng.integers(0, 2, n)]
    warps = []
    for k in range(n):
        kind = int(rng.integers(0, 5))
        if kind == 0:
            warps.append(None)
        elif kind == 1:
            warps.append(WR.rotate_matrix(float(rng.uniform(-40, 40)), SIZE, translate=(float(rng.uniform(-3, 3)), float(rng.uniform(-3, 3)))))
        elif kind == 2:
            warps.append((float(rng.uniform(0.5, 1.5)), 0.0, float(rng.uniform(-5, 5)), 0.0, float(rng.uniform(0.5, 1.5)), float(rng.uniform(-5, 5))))
        elif kind == 3:
            warps.append((1.0, float(rng.uniform(-0.4, 0.4)), 0.0, float(rng.uniform(-0.4, 0.4)), 1.0, 0.0))
        else:
            warps.append((-1.0, 0.0, float(SIZE[0]), 0.0, 1.0, float(rng.uniform(-2, 2))))
    return wins, flips, warps


def want_u8(data, win, m, filt, flip=False):
    src, _eff, _g = RZ._p_source(data, None, None, win)
    r = F.resize(src, SIZE[0], SIZE[1], F.BILINEAR)
    return WR.warp(r[:, ::-1] if flip else r, WR.IDENTITY if m is None else m, WR.BILINEAR if filt == "bilinear" else WR.NEAREST, WFILL)


@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
def test_fresh_windows_flips_and_warps_keep_the_sub_batches(monkeypatch, capfd, filt):
    fs = files()
    fmt, ref_fmt = TN.fmt_of("float32")
    rng = np.random.default_rng(7)
    p = J.Pipeline(threads=4)
    try:
        for c in range(3):
            PW._env(monkeypatch, {})
            monkeypatch.setenv("JPGPU_PIPE_TRACE", "1")
            wins, flips, warps = fresh(rng, len(fs))
            capfd.readouterr()
            out = p.decode(fs, windows=wins, output_size=SIZE, tensor=fmt, flips=flips, warp=J.WarpOptions(filt, WFILL), warps=warps)
            trace = capfd.readouterr().err
            assert "sub-batch" in trace and "+warp" in p.kernel_path and p.kernel_path.endswith("+tensor")
            if c:
                assert "created" not in trace and "re-windowed in place" in trace, (c, trace[-600:])
            for i, data in enumerate(fs):
                assert not isinstance(out[i], Exception), (c, i, out[i])
                u8 = want_u8(data, wins[i], warps[i], filt, flips[i])
                want = T.bits(T.to_tensor(u8, T.table(ref_fmt, u8.shape[2]), False))
                assert np.array_equal(T.bits(out[i]), want), (c, i, wins[i], flips[i], warps[i])
        # the same windows and flips with other matrices only: kept as they are
        wins2, flips2, warps2 = wins, flips, fresh(rng, len(fs))[2]
        capfd.readouterr()
        out = p.decode(fs, windows=wins2, output_size=SIZE, tensor=fmt, flips=flips2, warp=J.WarpOptions(filt, WFILL), warps=warps2)
        trace = capfd.readouterr().err
        assert "created" not in trace and "re-windowed" not in trace and "kept" in trace, trace[-600:]
        for i, data in enumerate(fs):
            u8 = want_u8(data, wins2[i], warps2[i], filt, flips2[i])
            assert np.array_equal(T.bits(out[i]), T.bits(T.to_tensor(u8, T.table(ref_fmt, u8.shape[2]), False))), i
    finally:
        monkeypatch.delenv("JPGPU_PIPE_TRACE", raising=False)
        p.close()


def test_u8_output_identities_and_the_warp_switched_off(monkeypatch, capfd):
    fs = files()[:8]
    rng = np.random.default_rng(9)
    _w, _f, warps = fresh(rng, len(fs))
    p = J.Pipeline(threads=4)
    try:
        PW._env(monkeypatch, {})
        monkeypatch.setenv("JPGPU_PIPE_TRACE", "1")
        out = p.decode(fs, output_size=SIZE, warp=J.WarpOptions("bilinear", WFILL), warps=warps)
        for i, data in enumerate(fs):
            assert np.array_equal(out[i], want_u8(data, None, warps[i], "bilinear").reshape(-1)), i
        capfd.readouterr()
        out = p.decode(fs, output_size=SIZE, warp=J.WarpOptions("bilinear", WFILL))  # (no matrices: identities, set in place)
        assert "created" not in capfd.readouterr().err
        plain = [F.resize(RZ._p_source(d, None, None, None)[0], SIZE[0], SIZE[1], F.BILINEAR).reshape(-1) for d in fs]
        for i in range(len(fs)):
            assert np.array_equal(out[i], plain[i]), i
        out = p.decode(fs, output_size=SIZE)  # (off: the sub-batches of the output size alone, created anew)
        assert "created" in capfd.readouterr().err and "warp" not in p.kernel_path
        for i in range(len(fs)):
            assert np.array_equal(out[i], plain[i]), i
        out = p.decode(fs, output_size=SIZE, warp=J.WarpOptions("nearest", WFILL), warps=warps)  # (and on again, the other filter)
        assert "created" in capfd.readouterr().err
        for i, data in enumerate(fs):
            assert np.array_equal(out[i], want_u8(data, None, warps[i], "nearest").reshape(-1)), i
    finally:
        monkeypatch.delenv("JPGPU_PIPE_TRACE", raising=False)
        p.close()


def test_one_refused_matrix_fails_its_image_alone(monkeypatch):
    PW._env(monkeypatch, {})
    fs = files()[:6]
    good = WR.rotate_matrix(20, SIZE)
    warps = [good, (1.0, 0.0, 40000.0, 0.0, 1.0, 0.0), None, (float("nan"), 0, 0, 0, 1, 0), good, (16000.5, 0, 0, 0, 1, 0)]
    p = J.Pipeline(threads=4)
    try:
        out = p.decode(fs, output_size=SIZE, warp=J.WarpOptions("nearest", WFILL), warps=warps)
        for i in (1, 3, 5):
            assert isinstance(out[i], J.FormatError) and "warp" in str(out[i]), (i, out[i])
        for i in (0, 2, 4):
            assert np.array_equal(out[i], want_u8(fs[i], None, warps[i], "nearest").reshape(-1)), i
        assert p.timings()["images_ok"] == 3
    finally:
        p.close()


def test_warps_without_options_and_a_warp_without_an_output_size_decode_nothing(monkeypatch):
    PW._env(monkeypatch, {})
    fs = files()[:2]
    p = J.Pipeline(threads=4)
    try:
        for kwargs in ({}, {"output_size": SIZE}):
            with pytest.raises(J.FormatError, match="warp options"):
                p.decode(fs, warps=[None, WR.rotate_matrix(5, SIZE)], **kwargs)
            assert J._native.lib().jpgpu_pipeline_pixel_bytes(p._h, 0) == 0
        with pytest.raises(J.FormatError, match="output size"):
            p.decode(fs, warp=J.WarpOptions())
        with pytest.raises(ValueError):
            p.decode(fs, output_size=SIZE, warp=J.WarpOptions(), warps=[None])
        bad = J._native.WarpOptionsStruct()
        bad.filter = 2
        assert J._native.lib().jpgpu_pipeline_set_warp(p._h, C.byref(bad)) == J._native.ERR_FORMAT
        out = p.decode(fs)  # (and the pipeline goes on as ever)
        PW._check_call(p, fs, [None, None], out)
    finally:
        p.close()
