"""EXIF orientation from JPEG bytes (jpgpu_pipeline_set_exif_orientation) on the MI355X: files written by tools/baseline_encoder.py
with an APP1 EXIF segment spliced in behind SOI.  The expected value is the reference resample of tests/orient_ref.py (pinned to Pillow by
tests/golden/orient) of the oracle's whole decode, sliced by the call's window in ORIENTED coordinates, compared with np.array_equal."""
import struct

import numpy as np
import pytest

import filter_ref as F
import orient_ref as OR
import placement_ref as P
import test_gpu_pipeline_windows as PW
import test_gpu_resize as RZ

pytestmark = pytest.mark.gpu

J = None
SIZE = (33, 41)
GEOM = (97, 61)
PFILL = (114, 7, 200, 33)


@pytest.fixture(scope="module", autouse=True)
def _load():
    global J
    import jpeg_decoder_amd as pkg
    J = pkg
    PW.J = pkg
    RZ.J = pkg
    assert J.device_count() >= 1, "no MI355X visible: the HIP path has no CPU fallback"


def exif_blob(o, e="<"):
    """A TIFF header and an IFD0 of two entries, the orientation the second."""
    make = struct.pack(e + "HHI", 0x010F, 2, 4) + b"abc\0"
    tag = struct.pack(e + "HHIHH", 0x0112, 3, 1, o, 0)
    return (b"II" if e == "<" else b"MM") + struct.pack(e + "HI", 42, 8) + struct.pack(e + "H", 2) + make + tag + struct.pack(e + "I", 0)


def with_exif(data, blob):
    """The file with an APP1 segment "Exif\\0\\0" + blob behind SOI."""
    assert data[:2] == b"\xff\xd8"
    payload = b"Exif\0\0" + blob
    return data[:2] + b"\xff\xe1" + struct.pack(">H", len(payload) + 2) + payload + data[2:]


def base_files(n=8):
    """4:2:0 and gray baseline files of one geometry."""
    return [PW._file(("420", "gray")[k % 2], "base", GEOM, pic=k) for k in range(n)]


def oriented(files, ors):
    return [with_exif(d, exif_blob(o, "<" if k % 2 else ">")) if o is not None else d for k, (d, o) in enumerate(zip(files, ors))]


def want(data, o, win, size=SIZE, placement=None):
    src, _eff, _g = RZ._p_source(data, None, None, None)
    a = OR.orient(src, o)
    if win is not None:
        x, y, w, h = win
        a = np.ascontiguousarray(a[y:y + h, x:x + w])
    if placement is not None:
        return F.placed(a, *placement, size[0], size[1], PFILL).reshape(-1)
    return F.resize(a, size[0], size[1], F.BILINEAR).reshape(-1)


def windows_for(ors, k):
    """A window inside every oriented image (every image windowed: the set of windowed images repeats from call to call)."""
    out = []
    for i, o in enumerate(ors):
        ow, oh = OR.oriented_size(o or 1, *GEOM)
        out.append((1 + (i + k) % 5, 3 + (2 * i + k) % 4, ow - 9 - (i % 3), oh - 11 - (k % 3)))
    return out


def check(p, files, ors, wins, out, label):
    for i, data in enumerate(files):
        assert not isinstance(out[i], Exception), (label, i, out[i])
        o = ors[i] or 1
        win = None if wins is None else wins[i]
        w = want(data, o, win)
        assert np.array_equal(out[i], w), (label, i, o, win, np.nonzero(out[i] != w)[0][:8].tolist())
        assert p.orientation(i) == o, (label, i)
        ow, oh = OR.oriented_size(o, *GEOM)
        assert p.window(i) == (tuple(win) if win is not None else (0, 0, ow, oh)), (label, i, p.window(i))
        info = p.info(i)
        assert (info.width, info.height) == GEOM, (label, i, info)  # (the file's own size)


@pytest.mark.parametrize("device_entropy", [True, False], ids=["device-entropy", "host-entropy"])
def test_every_orientation_from_bytes(monkeypatch, device_entropy):
    PW._env(monkeypatch, {})
    ors = [1, 2, 3, 4, 5, 6, 7, 8, None, 6]
    base = base_files(len(ors))
    files = oriented(base, ors)
    p = J.Pipeline(threads=4)
    try:
        out = p.decode(files, output_size=SIZE, exif_orientation=True, device_entropy=device_entropy)
        assert "+orient+resize" in p.kernel_path, p.kernel_path
        t = p.timings()
        assert (t["images_device_entropy"] > 0) == device_entropy and t["images_ok"] == len(files), t
        check(p, files, ors, None, out, "unwindowed")
        wins = windows_for(ors, 0)
        wins[3] = None
        out = p.decode(files, windows=wins, output_size=SIZE, exif_orientation=True, device_entropy=device_entropy)
        check(p, files, ors, wins, out, "windowed")
    finally:
        p.close()


def test_a_kept_pipeline_with_other_orientations_on_every_call(monkeypatch, capfd):
    """The same geometry sequence three times with other orientations per call, fresh windows at the same orientations, then the option
    off: a kept sub-batch never resamples with the orientations, the arena layout or the tables of the call before."""
    PW._env(monkeypatch, {})
    monkeypatch.setenv("JPGPU_PIPE_TRACE", "1")
    base = base_files(8)
    calls = [[6, 1, 8, 3, 1, 5, 2, 7], [1, 6, 3, 8, 5, 1, 7, 2], [8, 8, 1, 1, 6, 6, 4, 4]]
    p = J.Pipeline(threads=4)
    try:
        for c, ors in enumerate(calls):
            files = oriented(base, ors)
            wins = windows_for(ors, c)
            capfd.readouterr()
            out = p.decode(files, windows=wins, output_size=SIZE, exif_orientation=True)
            trace = capfd.readouterr().err
            assert "created" in trace, (c, trace[-400:])  # (other orientations: never the kept batch)
            check(p, files, ors, wins, out, f"call {c}")
        # fresh windows at the orientations of the call before: set in place, through the orientations the batch holds
        wins = windows_for(ors, 7)
        capfd.readouterr()
        out = p.decode(files, windows=wins, output_size=SIZE, exif_orientation=True)
        trace = capfd.readouterr().err
        assert "created" not in trace and "re-windowed in place" in trace, trace[-400:]
        check(p, files, ors, wins, out, "re-windowed")
        # the same call again: kept as it is
        capfd.readouterr()
        out = p.decode(files, windows=wins, output_size=SIZE, exif_orientation=True)
        trace = capfd.readouterr().err
        assert "created" not in trace and "re-windowed" not in trace and "kept" in trace, trace[-400:]
        check(p, files, ors, wins, out, "kept")
        # the option off: the files' tags are ignored, the windows are windows of the files as stored
        plain_wins = windows_for([1] * 8, 2)
        out = p.decode(files, windows=plain_wins, output_size=SIZE)
        assert "orient" not in p.kernel_path
        check(p, files, [None] * 8, plain_wins, out, "off")
        ref = p.decode(base, windows=plain_wins, output_size=SIZE)
        for a, b in zip(out, ref):
            assert np.array_equal(a, b)
        # and on again
        out = p.decode(files, windows=wins, output_size=SIZE, exif_orientation=True)
        check(p, files, ors, wins, out, "on again")
    finally:
        monkeypatch.delenv("JPGPU_PIPE_TRACE", raising=False)
        p.close()


def test_all_upright_files_are_the_call_without_the_option(monkeypatch):
    PW._env(monkeypatch, {})
    base = base_files(6)
    files = oriented(base, [1, None, 1, None, 1, 1])
    p = J.Pipeline(threads=4)
    try:
        a = p.decode(files, output_size=SIZE)
        path = p.kernel_path
        b = p.decode(files, output_size=SIZE, exif_orientation=True)
        assert p.kernel_path == path and "orient" not in path
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    finally:
        p.close()


def test_damaged_exif_decodes_as_orientation_1(monkeypatch):
    PW._env(monkeypatch, {})
    base = base_files(6)
    good = exif_blob(6)
    blobs = [good[:8 + 2 + 12 + 7], good[:6], b"II*\0\xff\xff\xff\x7f", exif_blob(9), exif_blob(0, ">"), good.replace(b"\x12\x01\x03\x00", b"\x12\x01\x04\x00")]
    files = [with_exif(d, b) for d, b in zip(base, blobs)]
    for b in blobs:
        assert OR.exif_orientation(b) == 1 and J.exif_orientation(b) == 1
    p = J.Pipeline(threads=4)
    try:
        out = p.decode(files, output_size=SIZE, exif_orientation=True)
        check(p, files, [None] * 6, None, out, "damaged")
    finally:
        p.close()


def test_the_fit_takes_the_oriented_size(monkeypatch):
    PW._env(monkeypatch, {})
    ors = [6, 8, 1, 5]
    base = base_files(4)
    files = oriented(base, ors)
    size = (40, 40)
    p = J.Pipeline(threads=4)
    try:
        for fit, rule in ((J.Fit("shorter_side_crop", 40, PFILL), lambda w, h: P.fit_shorter_side_crop(w, h, 40, *size)),
                          (J.Fit("letterbox", 0, PFILL), lambda w, h: P.fit_letterbox(w, h, *size))):
            out = p.decode(files, output_size=size, fit=fit, exif_orientation=True)
            for i, data in enumerate(files):
                pl = tuple(rule(*OR.oriented_size(ors[i], *GEOM)))
                assert p.placement(i) == pl, (fit, i, p.placement(i), pl)
                assert (pl != tuple(rule(*GEOM))) == (ors[i] >= 5)
                assert np.array_equal(out[i], want(data, ors[i], None, size, pl)), (fit, i)
    finally:
        p.close()


def test_unwindowed_420_files_keep_the_entry_list_walk(monkeypatch):
    PW._env(monkeypatch, {})
    n = 16
    base = [PW._file("420", "base", (333, 200), pic=k % 8) for k in range(n)]
    ors = [(6, 3, 8, 2)[k % 4] for k in range(n)]
    files = oriented(base, ors)
    p = J.Pipeline(threads=4)
    try:
        p.decode(base, output_size=SIZE)
        t0, path0 = p.timings(), p.kernel_path
        out = p.decode(files, output_size=SIZE, exif_orientation=True)
        t1 = p.timings()
        assert p.kernel_path == path0.replace("+resize", "+orient+resize"), (p.kernel_path, path0)
        for k in ("images_device_entropy", "images_device_rejected", "images_entry_pixels", "images_windowed"):
            assert t0[k] == t1[k], (k, t0[k], t1[k])
        assert t1["images_entry_pixels"] == n and t1["images_windowed"] == 0, t1
        for i in (0, 1, 2, 3, n - 1):
            src = RZ._p_source(files[i], None, None, None)[0]
            assert np.array_equal(out[i], F.resize(OR.orient(src, ors[i]), SIZE[0], SIZE[1], F.BILINEAR).reshape(-1)), i
    finally:
        p.close()


def test_errors(monkeypatch):
    PW._env(monkeypatch, {})
    base = base_files(4)
    files = oriented(base, [6, 1, 6, 6])
    p = J.Pipeline(threads=4)
    try:
        with pytest.raises(J.FormatError, match="output size"):
            p.decode(files, exif_orientation=True)  # (nothing is decoded)
        # a window that fits the file as stored but not the oriented image fails its image alone
        w, h = GEOM
        wins = [(0, 0, w, h), (0, 0, w, h), (0, 0, h, w), None]
        out = p.decode(files, windows=wins, output_size=SIZE, exif_orientation=True)
        assert isinstance(out[0], J.FormatError) and "oriented" in str(out[0]), out[0]
        for i in (1, 2, 3):
            assert np.array_equal(out[i], want(files[i], (6, 1, 6, 6)[i], None)), i
    finally:
        p.close()
