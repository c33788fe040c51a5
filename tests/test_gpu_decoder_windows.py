"""Decoder.set_window on the MI355X: both decoder routes (retained coefficients through a one-image windowed batch for small and
progressive images, the one-image device-entropy pipeline for large sequential ones), with and without scale, against the oracle's
whole decode sliced on the host."""
import os
import sys

import numpy as np
import pytest

import oracle as O

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "tools"))
import baseline_encoder as BE  # noqa: E402

pytestmark = pytest.mark.gpu
J = None
GOLDEN = os.path.join(_ROOT, "tests", "golden")
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _load():
    global J
    import jpeg_decoder_amd as pkg
    J = pkg
    assert J.device_count() >= 1, "no MI355X visible: the HIP path has no CPU fallback"


def _data(name):
    if name not in _CACHE:
        if name == "1080p":
            _CACHE[name] = BE.synthetic_jpeg(1920, 1080, seed=77)
        elif name == "2160p":
            _CACHE[name] = BE.synthetic_jpeg(3840, 2160, seed=78)
        elif name == "2160p-restart":
            _CACHE[name] = BE.synthetic_jpeg(3840, 2160, seed=79, restart_interval=240)
        else:
            with open(os.path.join(GOLDEN, *name.split("/")), "rb") as f:
                _CACHE[name] = f.read()
    return _CACHE[name]


def _slice(d, win):
    W, H = (d.components[0].size_w, d.components[0].size_h) if d.ncomp == 1 else (d.width, d.height)
    x, y, w, h = win
    return d.pixels.reshape(H, W, d.ncomp)[y:y + h, x:x + w].reshape(-1), (W, H)


FILES = ["benches/tower.jpg", "benches/tower_grayscale.jpg", "benches/tower_progressive.jpg", "reftest/mozilla/jpg-cmyk-2.jpg", "benches/large_image.jpg",
         "1080p", "2160p", "2160p-restart"]


@pytest.mark.parametrize("scaled", [False, True], ids=["full", "scaled"])
@pytest.mark.parametrize("name", FILES)
def test_decoder_window_is_the_slice_of_the_whole_decode(name, scaled):
    data = _data(name)
    whole = O.decode(data)
    req = (-(-whole.width // 2) - 3, -(-whole.height // 2) - 3) if scaled else None  # -> the 1/2 scale
    want_full = O.decode(data, scale_to=req)
    _, (W, H) = _slice(want_full, (0, 0, 1, 1))
    if scaled:
        assert (W, H) != (whole.width, whole.height)
    wins = [(13, 5, W // 2 | 1, H // 2 | 1), (W // 4 // 16 * 16, H // 4 // 16 * 16, W // 2 // 16 * 16, H // 2 // 16 * 16), (W - 1, H - 1, 1, 1), (0, H // 3, W, 1),
            (0, 0, W, H)]
    for win in wins:
        d = J.Decoder(data)
        try:
            d.set_window(*win)
            if req:
                assert d.scale(*req) == (want_full.width, want_full.height)
            d.read_info()
            assert J._native.lib().jpgpu_decoder_output_bytes(d._h) == win[2] * win[3] * want_full.ncomp
            got = d.decode()
            want, _ = _slice(want_full, win)
            assert got.size == want.size and np.array_equal(got, want), (name, win, got.size, want.size)
            assert (d.info().width, d.info().height) == (want_full.width, want_full.height)
        finally:
            d.close()


def test_window_then_whole_image_again():
    data = _data("benches/tower.jpg")
    d = J.Decoder(data)
    try:
        d.set_window(13, 5, 101, 77)
        d.set_window(0, 0, 0, 0)
        assert np.array_equal(d.decode(), O.decode(data).pixels)
    finally:
        d.close()


@pytest.mark.parametrize("name", ["benches/tower.jpg", "1080p", "benches/tower_progressive.jpg"])
def test_window_outside_the_output_is_a_format_error(name):
    data = _data(name)
    whole = O.decode(data)
    for win, scale in [((whole.width - 10, 0, 11, 5), None), ((0, whole.height, 1, 1), None),
                       ((whole.width // 2, whole.height // 2, whole.width // 4, whole.height // 4), (whole.width // 2 - 3, whole.height // 2 - 3))]:
        d = J.Decoder(data)
        try:
            d.set_window(*win)
            if scale:
                d.scale(*scale)
            with pytest.raises(J.FormatError, match="window"):
                d.decode()
        finally:
            d.close()


def test_a_damaged_stream_keeps_its_status_with_a_window():
    data = _data("benches/tower.jpg")
    cut = data[: len(data) * 2 // 3]
    plain = J.Decoder(cut)
    windowed = J.Decoder(cut)
    try:
        windowed.set_window(13, 5, 101, 77)
        try:
            want = plain.decode()
        except J.Error as e:
            with pytest.raises(type(e)) as got:
                windowed.decode()
            assert str(got.value) == str(e)
        else:
            assert np.array_equal(windowed.decode(), want.reshape(512, 512, 3)[5:82, 13:114].reshape(-1))
    finally:
        plain.close()
        windowed.close()


@pytest.mark.parametrize("name", ["benches/tower.jpg", "1080p"])
def test_failed_windowed_decodes_leak_no_context(name, monkeypatch):
    """More failing decoders than there are contexts (JPGPU_MAX_CONCURRENT_DECODES defaults to 64), then as many good ones."""
    data = _data(name)
    whole = O.decode(data)
    W, H = whole.width, whole.height
    for k in range(200):
        d = J.Decoder(data if k % 2 else data[:400])  # a window outside the image / a valid window on a file cut inside its header
        try:
            d.set_window(W - 5 if k % 2 else 5, k % H, 6, 1)
            with pytest.raises(J.Error):
                d.decode()
        finally:
            d.close()
    for k in range(200):
        d = J.Decoder(data)
        try:
            win = (k % 50, (7 * k) % 90, 33 + k % 20, 21 + k % 9)
            d.set_window(*win)
            got = d.decode()
            want, _ = _slice(whole, win)
            assert np.array_equal(got, want), (k, win)
        finally:
            d.close()
