"""RGB output without a GPU: the numpy statement of the conversion (tests/rgb_ref.py) equals Pillow's convert("RGB")
— through the pinned golden file, and directly where Pillow imports — the flag's refusals that need no device come back through the C
ABI, and the new symbol, flag and Python arguments are declared, exported and bound."""
import ctypes as C
import hashlib
import inspect
import json
import os

import numpy as np
import pytest

import jpeg_decoder_amd as J
import resample_ref as R
import rgb_ref as G
import tensor_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "rgb", "pillow_cmyk_to_rgb.json")))


def _table_input():
    X, K = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    return np.ascontiguousarray(np.stack([X, X, X, K], axis=2))


def test_cmyk_table_matches_the_pinned_pillow_table():
    got = G.to_rgb(_table_input())
    assert got.shape == (256, 256, 3) and got.dtype == np.uint8
    assert hashlib.sha256(got.tobytes()).hexdigest() == GOLDEN["table_sha256"]
    X, K = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    assert np.array_equal(got[:, :, 0].astype(int), (2 * (255 - X) * (255 - K) + 255) // 510)  # (the closed form of the definition)
    assert (got[:, :, 0].astype(int) <= 255 - K).all()  # (md <= nk: no clamp)


def test_explicit_pixels_and_gray():
    px = GOLDEN["pixels"]
    assert len(px) >= 24
    ks = {p["cmyk"][3] for p in px}
    assert 0 in ks and 255 in ks and any(0 in p["cmyk"][:3] for p in px) and any(255 in p["cmyk"][:3] for p in px)
    a = np.array([p["cmyk"] for p in px], np.uint8).reshape(1, -1, 4)
    assert np.array_equal(G.to_rgb(a).reshape(-1, 3), np.array([p["rgb"] for p in px], np.uint8))
    g = np.arange(256, dtype=np.uint8).reshape(1, 256, 1)
    assert np.array_equal(G.to_rgb(g).reshape(256, 3), np.array(GOLDEN["gray"], np.uint8))
    rgb = np.random.default_rng(1).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    assert np.array_equal(G.to_rgb(rgb), rgb)


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: f"{c['W']}x{c['H']}x{c['C']}-{c['ow']}x{c['oh']}")
def test_convert_then_resize_matches_pillow_hashes(case):
    a = np.random.default_rng(case["seed"]).integers(0, 256, (case["H"], case["W"], case["C"]), dtype=np.uint8)
    got = R.resize(G.to_rgb(a), case["ow"], case["oh"])
    assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == case["sha256"]


def test_against_pillow_directly():
    Image = pytest.importorskip("PIL.Image")
    table = np.asarray(Image.fromarray(_table_input(), "CMYK").convert("RGB"))
    assert np.array_equal(G.to_rgb(_table_input()), table)
    rng = np.random.default_rng(7)
    a = rng.integers(0, 256, (31, 45, 4), dtype=np.uint8)
    want = np.asarray(Image.fromarray(a, "CMYK").convert("RGB").resize((20, 13), Image.BILINEAR))
    assert np.array_equal(R.resize(G.to_rgb(a), 20, 13), want)
    # the order matters: converting AFTER the resample is another image
    assert not np.array_equal(G.to_rgb(R.resize(a, 20, 13)), want)
    g = rng.integers(0, 256, (31, 45), dtype=np.uint8)
    want = np.asarray(Image.fromarray(g, "L").convert("RGB").resize((20, 13), Image.BILINEAR))
    assert np.array_equal(R.resize(G.to_rgb(g[:, :, None]), 20, 13), want)


def _gray_desc():
    comps, _ = J.make_components(16, 16, [(1, 1)])
    return J.image_desc(list(comps), [[1] * 64], 16, 16, "Grayscale")


def _create(fn, *args):
    h = C.c_void_p()
    st = fn(*args, C.byref(h))
    msg = bytes(J.lib().jpgpu_batch_last_error(h)).decode() if h else ""
    J.lib().jpgpu_batch_destroy(h)
    return st, msg


def test_flag_without_an_output_size_is_refused_before_any_device_is_touched():
    N = J._native
    assert N.BATCH_RGB_OUTPUT == 8
    lib = J.lib()
    arr = (N.ImageDesc * 1)(_gray_desc())
    st, msg = _create(lib.jpgpu_batch_create, 0, arr, 1, N.BATCH_RGB_OUTPUT)
    assert st == N.ERR_UNSUPPORTED and "output size" in msg, (st, msg)
    win = (N.Window * 1)(N.Window(0, 0, 8, 8))
    st, msg = _create(lib.jpgpu_batch_create_windowed, 0, arr, win, 1, N.BATCH_RGB_OUTPUT)
    assert st == N.ERR_UNSUPPORTED and "output size" in msg, (st, msg)
    with pytest.raises(J.UnsupportedError):
        J.Batch([_gray_desc()], rgb=True)


def test_tensor_format_is_checked_for_three_channels_of_a_gray_image():
    """With the flag a gray image has three planes: a bad std[2] is refused (it would pass without the flag: one channel), a bad std[3]
    is none of its business.  Both come back before any device is touched."""
    N = J._native
    lib = J.lib()
    arr = (N.ImageDesc * 1)(_gray_desc())

    def fmt(std):
        s = N.TensorFormatStruct()
        s.dtype, s.reserved = N.TENSOR_F32, 0
        for c in range(4):
            s.mean[c], s.std[c] = 0.5, std[c]
        return s

    st, msg = _create(lib.jpgpu_batch_create_tensor, 0, arr, None, 8, 8, C.byref(fmt((1.0, 1.0, 0.0, 1.0))), 1, N.BATCH_RGB_OUTPUT)
    assert st == N.ERR_FORMAT and "std" in msg, (st, msg)
    if J.device_count() == 0:  # (what passes the format check goes on to the device: elsewhere the GPU tests cover it)
        st, msg = _create(lib.jpgpu_batch_create_tensor, 0, arr, None, 8, 8, C.byref(fmt((1.0, 1.0, 1.0, 0.0))), 1, N.BATCH_RGB_OUTPUT)
        assert st != N.ERR_FORMAT, (st, msg)
        st, msg = _create(lib.jpgpu_batch_create_tensor, 0, arr, None, 8, 8, C.byref(fmt((1.0, 1.0, 0.0, 1.0))), 1, N.BATCH_DEFAULT)
        assert st != N.ERR_FORMAT, (st, msg)
    want = T.table(("float32", (0.5,) * 4, (1.0, 2.0, 3.0, 4.0)), 3)
    assert want.shape == (3, 256) and not np.array_equal(want[0], want[2])


def test_new_symbol_flag_and_python_arguments():
    h1 = open(os.path.join(ROOT, "include", "jpgpu.h")).read()
    h2 = open(os.path.join(ROOT, "include", "jpgpu_decoder.h")).read()
    assert "JPGPU_BATCH_RGB_OUTPUT = 8" in h1
    assert "int jpgpu_pipeline_set_rgb_output(jpgpu_pipeline *p, int on);" in h2
    J.build()
    lib = C.CDLL(J._native.LIB_PATH)
    assert hasattr(lib, "jpgpu_pipeline_set_rgb_output") and "jpgpu_pipeline_set_rgb_output" in J._native.exported_symbols()
    assert lib.jpgpu_pipeline_set_rgb_output(None, 1) == J._native.ERR_FORMAT
    assert inspect.signature(J.Batch.__init__).parameters["rgb"].default is False
    assert inspect.signature(J.Pipeline.decode).parameters["rgb"].default is False
    # (no field was added to the timings)
    assert J._native.PipelineTimings._fields_[-1][0] == "images_windowed"
