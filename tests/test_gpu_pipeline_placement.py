"""The fit of a Pipeline (jpgpu_pipeline_set_fit) on the MI355X: JPEG bytes in, every image placed in the output size by its own source
size — the evaluation transform Resize(256) + CenterCrop(224) and the letterbox.  The expected value is always tests/placement_ref.py on
the oracle's decode with the placement the plain-Python rule gives, compared with np.array_equal."""
import ctypes as C

import numpy as np
import pytest

import placement_ref as P
import rgb_ref as G
import tensor_ref as T
import test_gpu_pipeline_windows as PW
import test_gpu_resize as RZ
import test_gpu_tensor as TN

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


def rule(fit, w, h, size):
    if fit.mode == "shorter_side_crop":
        return P.fit_shorter_side_crop(w, h, fit.size, size[0], size[1])
    if fit.mode == "letterbox":
        return P.fit_letterbox(w, h, size[0], size[1])
    return (size[0], size[1], 0, 0)


def _check(p, files, wins, out, size, fit, scale=None, ct=None, fmt=None, flips=None, rgb=False, label=""):
    bad = []
    for i, data in enumerate(files):
        win = None if wins is None else wins[i]
        src, eff, (W, H, nc) = RZ._p_source(data, scale, ct, win)
        pl = rule(fit, eff[2], eff[3], size)
        got = out[i]
        if isinstance(got, Exception):
            bad.append((i, win, repr(got)))
            continue
        assert p.placement(i) == pl == J.fit_placement(fit, (eff[2], eff[3]), size), (label, i, p.placement(i), pl)
        u8 = P.place(G.to_rgb(src) if rgb else src, size[0], size[1], pl, fit.fill)
        if fmt is None:
            ok = np.array_equal(got, u8.reshape(-1))
        else:
            want = T.to_tensor(u8, T.table(fmt, u8.shape[2]), bool(flips[i]) if flips else False)
            ok = got.shape == want.shape and np.array_equal(T.bits(got), T.bits(want))
        if not ok:
            bad.append((i, win, (W, H, nc), pl))
        assert p.window(i) == eff, (label, i)
    assert not bad, (label, size, bad[:8], len(bad))


EVAL = dict(mode="shorter_side_crop", size=256)
ROUTES = ["host-compact", "device", "prog-device", "prog-host"]


@pytest.mark.parametrize("mode", ["shorter_side_crop", "letterbox"])
@pytest.mark.parametrize("route", ROUTES)
def test_pipeline_fit_routes(monkeypatch, route, mode):
    """The host, device-entropy and progressive routes; sizes 500 x 375, 375 x 500 and the small files; u8 and tensor with flips."""
    enc, kwargs, env = PW.ROUTES[route]
    fit = J.Fit(mode, size=64, fill=(114, 7, 200)) if mode == "shorter_side_crop" else J.Fit(mode, fill=(114, 114, 114))
    size = (56, 56) if mode == "shorter_side_crop" else (96, 64)
    files = [PW._file("420", enc, (500, 375)), PW._file("420", enc, (375, 500), pic=1), PW._file("444", enc, (161, 97)), PW._file("gray", enc, (50, 34)),
             PW._file("422", enc, (50, 34), pic=2), PW._file("420", enc, (161, 97), pic=3)]
    PW._env(monkeypatch, env)
    p = J.Pipeline(threads=4)
    try:
        out = p.decode(files, output_size=size, fit=fit, **kwargs)
        _check(p, files, None, out, size, fit, label=f"{route} {mode} u8")
        assert "+place+resize" in p.kernel_path or p.kernel_path == "mixed", p.kernel_path
        assert p.timings()["pixel_bytes"] == sum(o.size for o in out)
        tf, ref = TN.fmt_of("float32")
        flips = [k % 2 == 1 for k in range(len(files))]
        out = p.decode(files, output_size=size, fit=fit, tensor=tf, flips=flips, **kwargs)
        _check(p, files, None, out, size, fit, fmt=ref, flips=flips, label=f"{route} {mode} f32")
    finally:
        p.close()


def test_pipeline_evaluation_transform_with_scale_rgb_and_windows(monkeypatch):
    """`scale=(256, 256)` plus the fit is Pillow's draft followed by Resize(256) + CenterCrop(224); windows place the window's size; RGB
    output places gray files with the fill in RGB order; fresh windows on the second call re-place in place."""
    PW._env(monkeypatch, {})
    fit, size = J.Fit(**EVAL), (224, 224)
    files = [PW._file("420", "base", (500, 375)), PW._file("420", "base", (375, 500), pic=1), PW._file("gray", "base", (161, 97)), PW._file("444", "base", (161, 97), pic=2)]
    p = J.Pipeline(threads=4)
    try:
        out = p.decode(files, output_size=size, fit=fit, scale=(256, 256))
        _check(p, files, None, out, size, fit, scale=(256, 256), label="scale")
        box = J.Fit("letterbox", fill=(1, 2, 3))
        out = p.decode(files, output_size=size, fit=box, rgb=True)
        _check(p, files, None, out, size, box, rgb=True, label="rgb")
        for wins in ([(13, 5, 301, 177), (1, 1, 100, 333), (5, 3, 70, 50), None], [(100, 50, 77, 201), (3, 7, 300, 100), (50, 30, 33, 21), None]):
            out = p.decode(files, output_size=size, fit=fit, windows=wins)
            _check(p, files, wins, out, size, fit, label="windows")
    finally:
        p.close()


def test_fresh_windows_at_the_same_fit_are_set_in_place(monkeypatch, capfd):
    PW._env(monkeypatch, {})
    monkeypatch.setenv("JPGPU_PIPE_TRACE", "1")
    fit, size = J.Fit("letterbox", fill=(114, 114, 114)), (64, 64)
    files = [PW._file("420", "base", (333, 200), pic=k) for k in range(8)]
    p = J.Pipeline(threads=4)
    try:
        for c, wname in enumerate(["A", "C", "B"]):
            wins = PW._windows_set(wname, 8)
            capfd.readouterr()
            out = p.decode(files, output_size=size, fit=fit, windows=wins)
            trace = capfd.readouterr().err
            _check(p, files, wins, out, size, fit, label=f"call {c}")
            assert ("re-windowed in place" in trace) == (c > 0), (c, trace[-600:])
    finally:
        monkeypatch.delenv("JPGPU_PIPE_TRACE", raising=False)
        p.close()


def test_fit_switched_on_changed_and_off_between_calls(monkeypatch):
    PW._env(monkeypatch, {})
    files = [PW._file("420", "base", (333, 200), pic=k) for k in range(6)]
    size = (64, 48)
    p = J.Pipeline(threads=4)
    try:
        plain = p.decode(files, output_size=size)
        path0 = p.kernel_path
        RZ._p_check(p, files, None, plain, size)
        assert [p.placement(i) for i in range(6)] == [(64, 48, 0, 0)] * 6
        for fit in (J.Fit("shorter_side_crop", size=60), J.Fit("letterbox", fill=(9, 8, 7)), J.Fit("letterbox", fill=(1, 1, 1)), J.Fit("shorter_side_crop", size=30, fill=(4, 5, 6))):
            out = p.decode(files, output_size=size, fit=fit)
            _check(p, files, None, out, size, fit, label=repr(fit))
            assert "+place" in p.kernel_path
        for off in (None, J.Fit("stretch", fill=(3, 3, 3))):  # (switched off: the plain resized bytes and path return)
            out = p.decode(files, output_size=size, fit=off)
            assert p.kernel_path == path0
            for a, b in zip(out, plain):
                assert np.array_equal(a, b)
    finally:
        p.close()


def test_refused_rule_fails_alone_and_a_missing_output_size_fails_the_call(monkeypatch):
    PW._env(monkeypatch, {})
    import synth
    thin = PW.BE.encode_rgb(synth.synthetic_rgb(8, 4000, seed=3), 85, "444")
    good = PW._file("420", "base", (161, 97))
    fit = J.Fit(**EVAL)
    p = J.Pipeline(threads=4)
    try:
        files = [good, thin, good]
        out = p.decode(files, output_size=(224, 224), fit=fit)
        assert isinstance(out[1], J.FormatError) and "fit" in str(out[1]), out[1]
        assert p.placement(1) is None
        src, eff, _g = RZ._p_source(good, None, None, None)
        pl = P.fit_shorter_side_crop(eff[2], eff[3], 256, 224, 224)
        for k in (0, 2):  # (its neighbours decode)
            assert p.placement(k) == pl and np.array_equal(out[k], P.place(src, 224, 224, pl).reshape(-1)), k
        out = p.decode(files, output_size=(224, 224), fit=J.Fit("letterbox"))  # (the letterbox places it: one column)
        assert p.placement(1) == P.fit_letterbox(8, 4000, 224, 224) and not isinstance(out[1], Exception)
        with pytest.raises(J.FormatError, match="output size"):
            p.decode(files, fit=fit)
        lib = J._native.lib()
        bad = J._native.FitStruct()
        bad.mode = 7
        assert lib.jpgpu_pipeline_set_fit(p._h, C.byref(bad)) == J._native.ERR_FORMAT
        bad.mode, bad.size, bad.reserved = 1, 256, 5
        assert lib.jpgpu_pipeline_set_fit(p._h, C.byref(bad)) == J._native.ERR_FORMAT
    finally:
        p.close()


def test_download_and_gather_modes_return_the_canvas(monkeypatch):
    PW._env(monkeypatch, {})
    files = [PW._file("420", "base", (333, 200), pic=k) for k in range(5)] + [PW._file("gray", "base", (161, 97), pic=1)]
    fit, size = J.Fit("letterbox", fill=(114, 114, 114)), (96, 96)
    p = J.Pipeline(threads=4)
    try:
        a = p.decode(files, download=True, output_size=size, fit=fit)
        _check(p, files, None, a, size, fit, label="download=True")
        assert p.timings()["pixel_bytes"] == sum(x.size for x in a) == 5 * 96 * 96 * 3 + 96 * 96
        counts = p.decode(files, download="pinned", output_size=size, fit=fit)
        assert counts == [x.size for x in a]
        b = [p.pixels_host(i).copy() for i in range(len(files))]
        counts = p.decode(files, download=False, output_size=size, fit=fit)
        c = [p.download(i) for i in range(len(files))]
        g = p.decode(files, output_size=size, fit=fit, gather=True)
        for i in range(len(files)):
            assert np.array_equal(a[i], b[i]) and np.array_equal(a[i], c[i]) and np.array_equal(a[i], g[i]), i
    finally:
        p.close()


def test_64_mixed_files_through_the_evaluation_transform_to_f32(monkeypatch):
    """One call of 64 files of mixed sizes through the evaluation transform, normalised to f32: every image compared."""
    PW._env(monkeypatch, {})
    sizes = [(500, 375), (375, 500), (333, 200), (161, 97), (256, 256), (50, 34), (300, 301), (640, 480)]
    files = [PW._file("420" if k % 3 else "444", "base", sizes[k % len(sizes)], pic=k % 5) for k in range(64)]
    fit, size = J.Fit(**EVAL), (224, 224)
    tf, ref = TN.fmt_of("float32")
    flips = [k % 2 == 0 for k in range(64)]
    p = J.Pipeline(threads=4)
    try:
        out = p.decode(files, output_size=size, fit=fit, tensor=tf, flips=flips)
        assert all(o.shape == (3, 224, 224) and o.dtype == np.float32 for o in out)
        _check(p, files, None, out, size, fit, fmt=ref, flips=flips, label="64")
        assert p.timings()["images_ok"] == 64 and p.timings()["pixel_bytes"] == 64 * 3 * 224 * 224 * 4
    finally:
        p.close()
